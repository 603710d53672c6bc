"""Host side of the HIP path: device memory, NHWC views, weight packing and the plan.

PyTorch is plumbing here (device allocations, streams); every arithmetic step of the
forward pass is a kernel of libglsdet_hip.so reached through the C ABI (``_lib``).
"""
from __future__ import annotations

import ctypes as C
import json
import os
import threading
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import F16, F32, ACT, View, ConvChain, ConvDesc, check, nonlocal_workspace_floats

_TORCH_DT = {F16: torch.float16, F32: torch.float32}
_ESIZE = {F16: 2, F32: 4}
# `decode_mode` of the reference harness (drone/yolo.py:75-82) -> sigmoid mask of Engine.decode (bit 0 objectness, bit 1
# classes); the one table HipDetector.detect and the drone twin's decode functions share
DECODE_MODES = {"default": 3, "obj_sigmoid": 1, "no_sigmoid": 0, "cls_sigmoid": 2}


def ceil_to(v: int, m: int) -> int:
    return (v + m - 1) // m * m


class TView:
    """NHWC view into a device allocation (mirrors glsdet_view).  Strides in elements."""
    __slots__ = ("buf", "off", "n", "h", "w", "c", "sn", "sh", "sw", "dtype")

    def __init__(self, buf: torch.Tensor, off: int, n: int, h: int, w: int, c: int,
                 sn: int, sh: int, sw: int, dtype: int):
        self.buf, self.off = buf, off
        self.n, self.h, self.w, self.c = n, h, w, c
        self.sn, self.sh, self.sw, self.dtype = sn, sh, sw, dtype

    # ---- sub-views (no copies: this is how torch.cat / slicing of the reference is realised)
    def channels(self, c0: int, c1: int) -> "TView":
        assert 0 <= c0 < c1 <= self.c and c0 % 8 == 0, (c0, c1, self.c)
        return TView(self.buf, self.off + c0, self.n, self.h, self.w, c1 - c0, self.sn, self.sh, self.sw, self.dtype)

    def image(self, b: int) -> "TView":
        """the n = 1 view of image b"""
        assert 0 <= b < self.n
        return TView(self.buf, self.off + b * self.sn, 1, self.h, self.w, self.c, self.sn, self.sh, self.sw, self.dtype)

    def window(self, h0: int, h1: int, w0: int, w1: int) -> "TView":
        assert 0 <= h0 < h1 <= self.h and 0 <= w0 < w1 <= self.w
        return TView(self.buf, self.off + h0 * self.sh + w0 * self.sw, self.n, h1 - h0, w1 - w0, self.c,
                     self.sn, self.sh, self.sw, self.dtype)

    def as_c(self) -> View:
        es = _ESIZE[self.dtype]
        lo = self.buf.data_ptr()
        return View(lo + self.off * es, self.sn, self.sh, self.sw, self.n, self.h, self.w, self.c,
                    self.dtype, 0, lo, lo + self.buf.numel() * self.buf.element_size())

    def to_nchw(self, c: Optional[int] = None) -> torch.Tensor:
        """Materialise as a dense NCHW fp32 torch tensor (tests / the drop-in surface)."""
        t = torch.as_strided(self.buf.view(_TORCH_DT[self.dtype]), (self.n, self.h, self.w, self.c),
                             (self.sn, self.sh, self.sw, 1), self.off)
        t = t[..., : (c or self.c)]
        return t.permute(0, 3, 1, 2).float().contiguous()

    def __repr__(self):
        return "TView[%d,%d,%d,%d %s]" % (self.n, self.h, self.w, self.c, "f16" if self.dtype == F16 else "f32")


class Plan:
    """Recorded op sequence (glsdet_plan): eager replay, hipGraph capture/replay, timing."""

    def __init__(self, lib):
        self.lib = lib
        self.h = lib.glsdet_plan_create()
        self.captured = False

    def __del__(self):
        try:
            if self.h:
                self.lib.glsdet_plan_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def __enter__(self):
        check(self.lib.glsdet_plan_begin(self.h), "plan_begin")
        return self

    def __exit__(self, *exc):
        check(self.lib.glsdet_plan_end(self.h), "plan_end")
        return False

    @property
    def num_ops(self) -> int:
        return self.lib.glsdet_plan_num_ops(self.h)

    def ops(self):
        out = []
        name = C.create_string_buffer(160)
        kind, fl, by = C.c_int32(), C.c_double(), C.c_double()
        for i in range(self.num_ops):
            check(self.lib.glsdet_plan_op_info(self.h, i, C.byref(kind), C.byref(fl), C.byref(by), name, 160))
            out.append({"kind": kind.value, "flops": fl.value, "bytes": by.value, "name": name.value.decode()})
        return out

    def run(self, stream=None):
        check(self.lib.glsdet_plan_run(self.h, _stream_ptr(stream)), "plan_run")

    def capture(self, stream):
        check(self.lib.glsdet_plan_capture(self.h, _stream_ptr(stream)), "plan_capture")
        self.captured = True

    def launch(self, stream=None):
        check(self.lib.glsdet_plan_launch(self.h, _stream_ptr(stream)), "plan_launch")

    def run_timed(self, stream=None, reps: int = 1) -> np.ndarray:
        ms = (C.c_float * self.num_ops)()
        for _ in range(reps):
            check(self.lib.glsdet_plan_run_timed(self.h, _stream_ptr(stream), ms), "plan_run_timed")
        return np.asarray(ms[:], np.float64) / reps


def _stream_ptr(stream) -> int:
    if stream is None:
        stream = torch.cuda.current_stream()
    return stream.cuda_stream


_SHARED_TUNED: dict = {}
_TUNE_IO_LOCK = threading.Lock()       # save_tune_cache: lanes of one process share the table and the cache file


def _in_geo(x: "TView") -> tuple:
    """sizes and strides of a view: the input part of a tune-cache key"""
    return (x.n, x.h, x.w, x.c, x.sn, x.sh, x.sw)


def _out_geo(o: "TView") -> tuple:
    """the output part of a tune-cache key (its n, h, w follow from the input and the conv)"""
    return (o.c, o.sn, o.sh, o.sw)


def _conv_desc(x: "TView", packed, stride: int, pad: int, act: str, out: "TView", res: Optional["TView"] = None,
               tile_hint: int = 0, res_first: bool = False, d: Optional[ConvDesc] = None) -> ConvDesc:
    """The glsdet_conv_desc of one conv (kernel size from `packed`); d: the struct to fill, an element of a ConvDesc array."""
    d = ConvDesc() if d is None else d
    d.x, d.y = x.as_c(), out.as_c()
    d.res = res.as_c() if res is not None else View()
    d.w, d.scale, d.bias = packed[0].data_ptr(), packed[1].data_ptr(), packed[2].data_ptr()
    d.R, d.S, d.stride, d.pad, d.act, d.tile_hint = packed[4], packed[5], stride, pad, ACT[act], tile_hint
    if res_first and res is not None:
        d.act |= 0x100                          # GLSDET_ACT_RES_FIRST
    return d


def _fused_loses(us: float, parts) -> bool:
    """The tuner's verdict on a fused launch of `us` microseconds against the launches it replaces (parts: their microseconds,
    each tuned on its own): it must come within 3 % of their sum, plus the credit for the launch it removes.  `parts` is
    consumed lazily; a part the tuner refused (None) ends the comparison and keeps the fused form."""
    total = 0.0
    for u in parts:
        if u is None:
            return False
        total += u
    return us > 0.97 * total + _fuse_credit_us()


class _Ptr:
    """device address with the .data_ptr() of a tensor (a weight operand that lives in an activation buffer)"""

    def __init__(self, ptr: int):
        self._p = ptr

    def data_ptr(self) -> int:
        return self._p


def expand_grouped_weight(w: torch.Tensor, groups: int) -> torch.Tensor:
    """grouped weights [C, Cg, R, S] -> the block-diagonal dense [C, C, R, S] (zeros outside each group's Cg x Cg block)"""
    c, cg = w.shape[0], w.shape[1]
    assert c == groups * cg, (tuple(w.shape), groups)
    dense = torch.zeros(c, c, w.shape[2], w.shape[3], dtype=w.dtype)
    for g in range(groups):
        dense[g * cg:(g + 1) * cg, g * cg:(g + 1) * cg] = w[g * cg:(g + 1) * cg]
    return dense


class GroupedPack:
    """Weights of one grouped 3x3 conv (Engine.pack_conv_grouped), uploaded in the form that is asked for, once:
    blocks() -- the `packed` tuple of the grouped kernel, None where it refuses the group width; dense() -- the `packed` tuple
    of the block-diagonal dense conv.  The engine that made it owns the uploads.  The fp32 host weights stay: either form may
    still be asked for (another geometry's tuner verdict, the shadow check)."""

    def __init__(self, eng: "Engine", w: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, groups: int):
        c, cg, R, S = w.shape
        assert (R, S) == (3, 3) and c == groups * cg and c % 8 == 0, (tuple(w.shape), groups)
        self.eng, self.groups, self.c, self.cg = eng, groups, c, cg
        self.kernel_takes = eng.lib.glsdet_conv_grouped_weight_elems(groups, cg) > 0
        self._host = (w, scale, bias)
        self._blocks = self._dense = None

    def blocks(self):
        if self._blocks is None and self.kernel_takes:
            from .torch_ops import grouped_weight_blocks
            w, scale, bias = self._host
            cpad = ceil_to(self.c, 32)
            sc, bi = torch.ones(cpad), torch.zeros(cpad)
            sc[:self.c], bi[:self.c] = scale, bias
            up = self.eng.upload
            self._blocks = (up(grouped_weight_blocks(w).to(_TORCH_DT[self.eng.dt])), up(sc), up(bi), self.c, 3, 3)
        return self._blocks

    def dense(self, keep: bool = True):
        """keep=False: a pack the CALLER owns (a tuner comparison holds it while it measures); adopt() makes it the cached one"""
        if self._dense is not None:
            return self._dense
        w, scale, bias = self._host
        pk = self.eng.pack_conv([(expand_grouped_weight(w, self.groups), scale, bias)], self.c, keep=keep)
        if keep:
            self._dense = pk
        return pk

    def adopt(self, pk):
        if self._dense is None:
            self.eng.keep(pk[:3])
            self._dense = pk


class Engine:
    """Owns device buffers and packed weights; emits ops (eagerly or into a Plan)."""

    def __init__(self, dtype: str = "f16", device: str = "cuda:0", autotune: bool = False):
        self.lib = _lib.load()          # raises GlsdetLibraryError when the .so is missing
        if not torch.cuda.is_available():
            raise _lib.GlsdetLibraryError("glsdet_amd needs an MI355X visible to PyTorch-ROCm (no CPU fallback)")
        assert dtype in ("f16", "f32")
        self.dt = F16 if dtype == "f16" else F32
        self.device = torch.device(device)
        self.stream = None              # None -> torch current stream at call time
        self._keep: List[torch.Tensor] = []
        self.alloc_bytes = 0
        self.autotune = autotune        # measure kernel/tile variants per conv problem at build time
        # tuning results are shared by all engines of a dtype in this process: the second and third
        # plan instance of a detector reuse the first one's measurements (and pick identical kernels)
        self._tuned = _SHARED_TUNED.setdefault(dtype, {})
        # optional persistent tuning cache (JSON): GLSDET_TUNE_CACHE=/path/file.json
        self._tune_cache_path = os.environ.get("GLSDET_TUNE_CACHE", "")
        if self._tune_cache_path and os.path.exists(self._tune_cache_path):
            with open(self._tune_cache_path) as f:
                self._tuned.update({tuple(json.loads(k)): v for k, v in json.load(f).get(dtype, {}).items()})
        self._tune_dirty = False        # save_tune_cache has something to write
        self._dtype_name = dtype
        self._vecs: dict = {}
        # verification (tools/variant_check.py): {"hint": h, "multi": h or None, "log": []} -- every conv also runs
        # on kernel variant h into a scratch tensor (same operands, before the real launch) and the two results are
        # compared element by element; eager emission only
        self.shadow = None

    # ---- memory
    def raw(self, nbytes: int) -> torch.Tensor:
        t = torch.zeros(ceil_to(max(nbytes, 16), 256), dtype=torch.uint8, device=self.device)
        self._keep.append(t)
        self.alloc_bytes += t.numel()
        return t

    def tensor(self, n: int, h: int, w: int, c: int, dtype: Optional[int] = None) -> TView:
        dt = self.dt if dtype is None else dtype
        cp = ceil_to(c, 8)
        buf = self.raw(n * h * w * cp * _ESIZE[dt])
        return TView(buf, 0, n, h, w, cp, h * w * cp, w * cp, cp, dt)

    def upload(self, arr: torch.Tensor, keep: bool = True) -> torch.Tensor:
        """keep=False: the caller owns the device tensor (it is freed with the caller's last reference)"""
        t = arr.contiguous().to(self.device)
        if keep:
            self.keep([t])
        return t

    def keep(self, tensors) -> None:
        for t in tensors:
            self._keep.append(t)
            self.alloc_bytes += t.numel() * t.element_size()

    # ---- weights
    def pack_conv(self, parts: Sequence[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]], cin_pad: int, keep: bool = True):
        """parts: [(w OIHW fp32, scale[O], bias[O])...] concatenated along O.
        -> (w_dev [cout_pad][kpad] in engine dtype, scale_dev, bias_dev, cout, R, S); keep: as Engine.upload"""
        w = torch.cat([p[0].float() for p in parts], 0)
        scale = torch.cat([p[1].float() for p in parts], 0)
        bias = torch.cat([p[2].float() for p in parts], 0)
        cout, cin, R, S = w.shape
        assert cin <= cin_pad and cin_pad % 8 == 0
        kpad = self.lib.glsdet_conv_kpad(R, S, cin_pad, self.dt)
        cpad = self.lib.glsdet_conv_cout_pad(ceil_to(cout, 8))
        wp = torch.zeros(cpad, R, S, cin_pad, dtype=torch.float32)
        wp[:cout, :, :, :cin] = w.permute(0, 2, 3, 1)
        flat = torch.zeros(cpad, kpad, dtype=torch.float32)
        flat[:, : R * S * cin_pad] = wp.reshape(cpad, -1)
        sc = torch.ones(cpad, dtype=torch.float32)
        bi = torch.zeros(cpad, dtype=torch.float32)
        sc[:cout], bi[:cout] = scale, bias
        return (self.upload(flat.to(_TORCH_DT[self.dt]), keep), self.upload(sc, keep), self.upload(bi, keep), cout, R, S)

    # ---- the tuner
    def _tune(self, key: tuple, measure) -> int:
        """the tune table's entry for `key`; a miss stores what measure() returns"""
        if key not in self._tuned:
            self._tuned[key] = measure()
            self._tune_dirty = True
        return self._tuned[key]

    def _measure(self, tune_fn, *args, must: str = ""):
        """one `*_tune` entry point -> (rc, best variant, its microseconds); must: raise under that name when it refuses"""
        best, us = C.c_int32(0), C.c_float(0)
        rc = tune_fn(*args, _stream_ptr(self.stream), C.byref(best), C.byref(us))
        if must:
            check(rc, must)
        return rc, best.value, us.value

    def _conv_us(self, d: ConvDesc) -> Optional[float]:
        """microseconds of the plain conv d on its best variant (glsdet_conv2d_tune), None when the tuner refuses it"""
        rc, _, us = self._measure(self.lib.glsdet_conv2d_tune, C.byref(d))
        return us if rc == 0 else None

    # ---- ops (each is one C-ABI call)
    def conv(self, x: TView, packed, stride: int, pad: int, act: str, out: Optional[TView] = None,
             res: Optional[TView] = None, out_dtype: Optional[int] = None, tile_hint: int = 0,
             res_first: bool = False) -> TView:
        """res_first: act(conv*scale + bias + res) (ResNet) instead of act(conv*scale + bias) + res."""
        cout, R, S = packed[3:]
        ho = (x.h + 2 * pad - R) // stride + 1
        wo = (x.w + 2 * pad - S) // stride + 1
        if out is None:
            out = self.tensor(x.n, ho, wo, cout, out_dtype)
        assert out.c == ceil_to(cout, 8), (out.c, cout)
        d = _conv_desc(x, packed, stride, pad, act, out, res, tile_hint, res_first)
        if self.autotune and tile_hint == 0:
            key = _in_geo(x) + _out_geo(out) + (R, S, stride, pad, res is not None, out.dtype)
            d.tile_hint = self._tune(key, lambda: self._measure(self.lib.glsdet_conv2d_tune, C.byref(d), must="conv2d_tune")[1])
        sh = None
        if self.shadow is not None and tile_hint == 0 and self.shadow.get("hint"):
            sh = self._shadow_begin([d], [out], self.shadow["hint"], multi=False)
        forced = os.environ.get("GLSDET_FORCE_HINT")          # verification runs: every conv uses this variant
        if forced and tile_hint == 0:                          # wherever it accepts the problem
            d.tile_hint = int(forced, 0)
            if self.lib.glsdet_conv2d(C.byref(d), _stream_ptr(self.stream)) == 0:
                return out
            d.tile_hint = 0
        check(self.lib.glsdet_conv2d(C.byref(d), _stream_ptr(self.stream)), "conv2d")
        self._shadow_end(sh)
        return out

    def conv_chain(self, x: TView, packed, stride: int, pad: int, act: str, out: TView, res: Optional[TView],
                   packed2, act2: str, c0: int, cin2: int, out2: TView, res_first: bool = False, skip_y: bool = False) -> bool:
        """conv (as Engine.conv) + in the same launch a 1x1 conv (packed2, act2) on channels [c0, c0 + cin2) of its result
        -> out2 (glsdet_conv2d_chain).  Returns False, having launched nothing, when no kernel takes the fused problem
        (the caller then emits the two convs).  skip_y: nothing else reads `out` -- it is not stored (GLSDET_CHAIN_SKIP_Y;
        `out` is then only a scratch view for the tuner's comparison and the shadow check)."""
        R, S = packed[4:]
        w2, s2, b2, cout2, R2, S2 = packed2
        assert R2 == 1 and S2 == 1 and out2.c == ceil_to(cout2, 8)
        d = _conv_desc(x, packed, stride, pad, act, out, res, res_first=res_first)
        c = ConvChain()
        c.y2 = out2.as_c()
        c.w2, c.scale2, c.bias2 = w2.data_ptr(), s2.data_ptr(), b2.data_ptr()
        c.act2, c.c0, c.cin2 = ACT[act2], c0, cin2
        c.flags = 1 if skip_y else 0
        st = _stream_ptr(self.stream)
        if self.autotune:
            key = ("chain",) + _in_geo(x) + _out_geo(out) + (R, S, stride, pad, res is not None, out.dtype, c0, c.cin2) + \
                _out_geo(out2) + (bool(skip_y),)

            def measure():
                rc, best, us = self._measure(self.lib.glsdet_conv2d_chain_tune, C.byref(d), C.byref(c))
                hint = best if rc == 0 else -1
                if hint >= 0:
                    # fused only where it beats the two launches it replaces (each tuned on its own): the chained product
                    # runs in the tail of the producing workgroups, which costs more than a launch on some shapes
                    d2 = _conv_desc(out.channels(c0, c0 + cin2), packed2, 1, 0, act2, out2)
                    if _fused_loses(us, (self._conv_us(dd) for dd in (d, d2))):
                        hint = -1
                return hint

            d.tile_hint = self._tune(key, measure)
            if d.tile_hint < 0:
                return False
        sh = None
        if self.shadow is not None and self.shadow.get("hint") and not skip_y:   # the variant under test computes y (unfused) first
            sh = self._shadow_begin([d], [out], self.shadow["hint"], multi=False)
        ok = self.lib.glsdet_conv2d_chain(C.byref(d), C.byref(c), st) == 0
        if ok and self.shadow is not None:
            self._shadow_end(sh)
            if skip_y:                                # y was not stored: produce it for the stand-alone 1x1 of the check below
                self.conv(x, packed, stride, pad, act, out=out, tile_hint=1)
            # and the chained product against a stand-alone 1x1 on the stored y: bit for bit
            ref = self.tensor(out2.n, out2.h, out2.w, out2.c, out2.dtype)
            self.conv(out.channels(c0, c0 + cin2), packed2, 1, 0, act2, out=ref, tile_hint=1)
            self._shadow_record((x.n, out.h, out.w, cin2, out2.c, 1, 1), out2, ref)
        return ok

    def bottleneck(self, x: TView, packed1, act1: str, packed2, act2: str, out: TView, res: Optional[TView],
                   hidden: TView) -> bool:
        """y = act2(conv3x3(act1(conv1x1(x)))) (+ res) in ONE launch (glsdet_bottleneck): the 1x1 is recomputed on the
        halo of the 3x3's tiles and the hidden tensor never exists in memory.  `out` must not alias x.  Returns False,
        having launched nothing, when the fused kernel does not apply or (autotune) does not beat the two tuned launches
        it replaces; `hidden` is the scratch tensor the comparison (and the caller's fallback) uses."""
        (cm, R1, S1), (cout, R2, S2) = packed1[3:], packed2[3:]
        if (R1, S1, R2, S2) != (1, 1, 3, 3) or cm != cout or cm not in (32, 64, 128) or x.dtype != out.dtype:
            return False
        d1 = _conv_desc(x, packed1, 1, 0, act1, hidden)
        d2 = _conv_desc(hidden, packed2, 1, 1, act2, out, res)
        hint = 0
        if self.autotune:
            key = ("bneck",) + _in_geo(x) + (cm,) + _out_geo(out)[1:] + (res is not None, out.dtype)

            def measure():
                rc, best, us = self._measure(self.lib.glsdet_bottleneck_tune, C.byref(d1), C.byref(d2))
                hint = best if rc == 0 else -1
                # against the two launches it replaces, each tuned on its own
                if hint >= 0 and _fused_loses(us, (self._conv_us(dd) for dd in (d1, d2))) and not os.environ.get("GLSDET_FORCE_BNECK"):
                    hint = -1
                return hint

            hint = self._tune(key, measure)
            if hint < 0:
                return False
        ok = self.lib.glsdet_bottleneck(C.byref(d1), C.byref(d2), hint, _stream_ptr(self.stream)) == 0
        if ok and self.shadow is not None:      # against the two-launch form on the same operands: bit for bit
            ref = self.tensor(out.n, out.h, out.w, out.c, out.dtype)
            self.conv(x, packed1, 1, 0, act1, out=hidden, tile_hint=1)
            self.conv(hidden, packed2, 1, 1, act2, out=ref, res=res, tile_hint=1)
            self._shadow_record((x.n, out.h, out.w, cm, cm, 3, 3), out, ref)
        return ok

    # ---- a whole CSPLayer (64 -> 64, hidden 32, one Bottleneck) as ONE launch (glsdet_csp_fused)
    def _tmp(self, n: int, h: int, w: int, c: int, sn: Optional[int] = None, sh: Optional[int] = None,
             sw: Optional[int] = None) -> TView:
        """a view on a buffer of its own that is freed with it (tuner comparisons, shadow checks)"""
        sw = c if sw is None else sw
        sh = w * sw if sh is None else sh
        sn = h * sh if sn is None else sn
        buf = torch.zeros(ceil_to(n * sn * _ESIZE[self.dt], 256), dtype=torch.uint8, device=self.device)
        return TView(buf, 0, n, h, w, c, sn, sh, sw, self.dt)

    def _csp_desc(self, x: TView, out: TView, packs, shortcut: bool) -> "_lib.CspDesc":
        d = _lib.CspDesc()
        d.x, d.y = x.as_c(), out.as_c()
        for q, pk in zip(("12", "m1", "m2", "3"), packs):
            setattr(d, "w" + q, pk[0].data_ptr())
            setattr(d, "scale" + q, pk[1].data_ptr())
            setattr(d, "bias" + q, pk[2].data_ptr())
        d.act, d.shortcut = ACT["silu"], 1 if shortcut else 0
        return d

    def _csp_unfused(self, x: TView, packs, shortcut: bool, out: TView, launch) -> None:
        """the four launches glsdet_csp_fused replaces, on buffers of their own; launch(x, pack, pad, out, res)"""
        cat = self._tmp(x.n, x.h, x.w, 64)
        t = self._tmp(x.n, x.h, x.w, 32)
        main = cat.channels(0, 32)
        launch(x, packs[0], 0, cat, None)
        launch(main, packs[1], 0, t, None)
        launch(t, packs[2], 1, main, main if shortcut else None)
        launch(cat, packs[3], 0, out, None)

    def _csp_key(self, xg, og, shortcut: bool) -> tuple:
        """tune-cache key of the fused CSPLayer; xg / og = (n, h, w, c, sn, sh, sw) of its input / output view"""
        return ("csp1",) + tuple(int(v) for v in xg) + tuple(int(v) for v in og) + (bool(shortcut), int(self.dt))

    def csp_fused_wins(self, xg, og, packs, shortcut: bool) -> bool:
        """Would Engine.csp_fused take the layer?  xg / og = (n, h, w, c, sn, sh, sw) of its input / output view (the input
        may not exist yet: the caller decides BEFORE it emits the layer's producer); packs = the packed convs conv1|conv2,
        m.0.conv1, m.0.conv2, conv3.  Records no op.  Without autotune: wherever the entry point accepts the operands.  With
        autotune the fused launch must beat the four tuned launches it replaces (each timed by glsdet_conv2d_tune on
        buffers of its own; only the key ("csp1", ...) is stored)."""
        if self.dt != F16 or xg[3] != 64 or og[3] != 64 or tuple(xg[:3]) != tuple(og[:3]) or len(packs) != 4 or \
                [(pk[3], pk[4], pk[5]) for pk in packs] != [(64, 1, 1), (32, 1, 1), (32, 3, 3), (64, 1, 1)]:
            return False
        if not self.autotune:
            return True

        def measure():
            x, out = self._tmp(*xg), self._tmp(*og)
            rc, best, us = self._measure(self.lib.glsdet_csp_fused_tune, C.byref(self._csp_desc(x, out, packs, shortcut)))
            hint = best if rc == 0 else -1
            if hint >= 0:
                sep = []            # all four are timed, also after one was refused
                self._csp_unfused(x, packs, shortcut, out, lambda xi, pk, pad, o, res:
                                  sep.append(self._conv_us(_conv_desc(xi, pk, 1, pad, "silu", o, res))))
                if _fused_loses(us, sep):
                    hint = -1
            return hint

        return self._tune(self._csp_key(xg, og, shortcut), measure) >= 0

    def csp_fused(self, x: TView, packs, shortcut: bool, out: TView) -> bool:
        """The CSPLayer x -> out in ONE launch (glsdet_csp_fused; packs as for csp_fused_wins): bit-identical to the four
        launches.  Returns False, having launched nothing, when the entry point refuses the operands."""
        hint = max(self._tuned.get(self._csp_key(_in_geo(x), _in_geo(out), shortcut), 0), 0) if self.autotune else 0
        d = self._csp_desc(x, out, packs, shortcut)
        ok = self.lib.glsdet_csp_fused(C.byref(d), hint, _stream_ptr(self.stream)) == 0
        if ok and self.shadow is not None:      # against the four-launch form on the same operands: bit for bit
            ref = self._tmp(out.n, out.h, out.w, out.c)
            self._csp_unfused(x, packs, shortcut, ref,
                              lambda xi, pk, pad, o, res: self.conv(xi, pk, 1, pad, "silu", out=o, res=res, tile_hint=1))
            self._shadow_record((x.n, out.h, out.w, 64, 64, 3, 3), out, ref)
        return ok

    def conv_multi(self, xs: Sequence[TView], packs, stride: int, pad: int, act: str,
                   outs: Optional[Sequence[Optional[TView]]] = None, ress: Optional[Sequence[Optional[TView]]] = None,
                   out_dtype: Optional[int] = None, tile_hint: int = 0) -> List[TView]:
        """Up to 8 independent convs of one shape class (same k, stride, Cin, Cout) as ONE launch
        (glsdet_conv2d_multi): each alone is too small to fill the chip."""
        n = len(xs)
        assert 1 <= n <= 32 and len(packs) == n
        outs = list(outs) if outs is not None else [None] * n
        ress = list(ress) if ress is not None else [None] * n
        arr = (ConvDesc * n)()
        for i, (x, pk) in enumerate(zip(xs, packs)):
            cout, R, S = pk[3:]
            if outs[i] is None:
                outs[i] = self.tensor(x.n, (x.h + 2 * pad - R) // stride + 1, (x.w + 2 * pad - S) // stride + 1, cout, out_dtype)
            _conv_desc(x, pk, stride, pad, act, outs[i], ress[i], tile_hint, d=arr[i])
        sh = None
        if self.shadow is not None and self.shadow.get("multi"):
            sh = self._shadow_begin([arr[i] for i in range(n)], outs, self.shadow["multi"], multi=True)
        forced = os.environ.get("GLSDET_FORCE_MULTI_HINT")
        if forced and tile_hint == 0:
            arr[0].tile_hint = int(forced, 0)
            if self.lib.glsdet_conv2d_multi(arr, n, _stream_ptr(self.stream)) == 0:
                return outs
            arr[0].tile_hint = 0
        check(self.lib.glsdet_conv2d_multi(arr, n, _stream_ptr(self.stream)), "conv2d_multi")
        self._shadow_end(sh)
        return outs

    def conv_many(self, xs: Sequence[TView], packs, stride: int, pad: int, act: str, outs: Sequence[TView],
                  ress: Optional[Sequence[Optional[TView]]] = None) -> List[TView]:
        """Any number of independent convs of one shape class: eight per launch, or -- 1x1 problems of ONE geometry (sizes,
        strides, residual or not: the per-window GEMMs of the ResNet GL plug-in) -- up to 32 per launch (the batched form of
        glsdet_conv2d_multi: one argument block + the operand addresses of each problem), on the tile the tuner measures."""
        ress = list(ress) if ress is not None else [None] * len(xs)
        n = len(xs)
        geo = lambda x, pk, o, r: _in_geo(x) + (x.dtype, pk[3], pk[4], pk[5]) + _in_geo(o) + (o.dtype,) + \
            ((-1, -1, -1, -1) if r is None else (r.sn, r.sh, r.sw, r.c))          # (flat: a tune-cache key)
        per = 8
        if n > 8 and stride == 1 and pad == 0 and packs[0][4] == 1 and packs[0][5] == 1 and not os.environ.get("GLSDET_NO_BATCH") and \
                len({geo(x, pk, o, r) for x, pk, o, r in zip(xs, packs, outs, ress)}) == 1:
            per = 32
        for i in range(0, n, per):
            k = min(per, n - i)
            hint = 0
            if k > 8 and self.autotune:
                def measure():
                    arr = (ConvDesc * k)()
                    for j in range(k):
                        _conv_desc(xs[i + j], packs[i + j], 1, 0, act, outs[i + j], ress[i + j], d=arr[j])
                    return self._measure(self.lib.glsdet_conv2d_multi_tune, arr, k, must="conv2d_multi_tune")[1]

                hint = self._tune(("batch", k, act) + geo(xs[i], packs[i], outs[i], ress[i]), measure)
            self.conv_multi(xs[i:i + k], packs[i:i + k], stride, pad, act, outs=outs[i:i + k], ress=ress[i:i + k], tile_hint=hint)
        return list(outs)

    def matrix(self, rows: int, cols: int, dtype: Optional[int] = None) -> TView:
        """Dense rows x cols matrix that can serve BOTH as a 1x1-conv activation (rows = pixels, cols = channels)
        and as a 1x1-conv weight operand (rows = output channels): row pitch = glsdet_conv_kpad(cols), rows padded
        to the weight tile granule (32), zero filled.  -> view [1, 1, rows, ceil8(cols)]."""
        dt = self.dt if dtype is None else dtype
        c8 = ceil_to(cols, 8)
        pitch = self.lib.glsdet_conv_kpad(1, 1, c8, dt)
        rp = self.lib.glsdet_conv_cout_pad(ceil_to(rows, 8))
        buf = self.raw(rp * pitch * _ESIZE[dt])
        return TView(buf, 0, 1, 1, rows, c8, rows * pitch, rows * pitch, pitch, dt)

    def bias_vector(self, n: int) -> TView:
        """fp32 vector of n entries (zero filled, padded to the weight row granule) that a 1-pixel conv of the plan writes
        and a later conv reads as its per-channel bias (as_weight(bias_dev=)): -> view [1, 1, 1, n]."""
        cpad = self.lib.glsdet_conv_cout_pad(ceil_to(n, 8))
        buf = self.raw(cpad * 4)
        return TView(buf, 0, 1, 1, 1, ceil_to(n, 8), cpad, cpad, cpad, F32)

    def as_weight(self, m: TView, alpha: float = 1.0, bias: Optional[torch.Tensor] = None, bias_dev: Optional[TView] = None):
        """`packed` tuple for Engine.conv whose weight operand is the activation matrix m (Engine.matrix layout):
        out[pixel][r] = alpha * sum_k x[pixel][k] * m[r][k] (+ bias[r]).  bias: host constant; bias_dev: an fp32 vector an
        earlier op of the plan writes (Engine.bias_vector)."""
        rows = m.h * m.w
        assert m.n == 1 and m.sw == self.lib.glsdet_conv_kpad(1, 1, m.c, m.dtype), "as_weight needs an Engine.matrix view"
        cpad = self.lib.glsdet_conv_cout_pad(ceil_to(rows, 8))
        assert bias_dev is None or (bias is None and bias_dev.dtype == F32 and bias_dev.sw >= cpad), \
            "bias_dev: Engine.bias_vector of >= cout_pad floats"
        key = ("vec", cpad, float(alpha))
        if key not in self._vecs:
            self._vecs[key] = (self.upload(torch.full((cpad,), float(alpha))), self.upload(torch.zeros(cpad)))
        sc, zero = self._vecs[key]
        if bias_dev is not None:
            zero = _Ptr(bias_dev.buf.data_ptr() + bias_dev.off * _ESIZE[F32])
        elif bias is not None:
            bkey = ("bias", cpad, bias.data_ptr())
            if bkey not in self._vecs:
                b = torch.zeros(cpad)
                b[: bias.numel()] = bias.float()
                self._vecs[bkey] = (self.upload(b), bias)        # keeps `bias` alive: its address is the key
            zero = self._vecs[bkey][0]
        return (_Ptr(m.buf.data_ptr() + m.off * _ESIZE[m.dtype]), sc, zero, ceil_to(rows, 8), 1, 1)

    def conv_group(self, xs: Sequence[TView], packs, stride: int, pad: int, act: str,
                   outs: Optional[Sequence[Optional[TView]]] = None, ress: Optional[Sequence[Optional[TView]]] = None,
                   out_dtype: Optional[int] = None) -> List[TView]:
        """n independent convs of one shape class: ONE grouped launch when that is faster than n
        launches (measured at build time with autotune, a size heuristic without), else n convs."""
        n = len(xs)
        outs = list(outs) if outs is not None else [None] * n
        ress = list(ress) if ress is not None else [None] * n
        R, S, cout = packs[0][4], packs[0][5], packs[0][3]
        for i, x in enumerate(xs):
            if outs[i] is None:
                outs[i] = self.tensor(x.n, (x.h + 2 * pad - R) // stride + 1, (x.w + 2 * pad - S) // stride + 1, cout, out_dtype)
        separate = lambda: [self.conv(x, pk, stride, pad, act, out=o, res=r, out_dtype=out_dtype)
                            for x, pk, o, r in zip(xs, packs, outs, ress)]
        if n < 2 or n > 4 or len({(pk[3], pk[4], pk[5], x.c) for x, pk in zip(xs, packs)}) != 1 or \
                os.environ.get("GLSDET_NO_GROUP"):          # A/B switch for measurements
            return separate()
        if not self.autotune:
            small = all(o.n * o.h * o.w * o.c <= 64 * 64 * 384 for o in outs)
            return self.conv_multi(xs, packs, stride, pad, act, outs=outs, ress=ress) if small else separate()
        key = ("multi", n, stride, pad, R, S) + tuple(v for x, o, r in zip(xs, outs, ress)
                                                      for v in _in_geo(x) + _out_geo(o) + (r is not None, o.dtype))

        def measure():
            arr = (ConvDesc * n)()
            single_us = 0.0
            for i, (x, pk, o, r) in enumerate(zip(xs, packs, outs, ress)):
                d = _conv_desc(x, pk, stride, pad, act, o, r, d=arr[i])
                single_us += self._measure(self.lib.glsdet_conv2d_tune, C.byref(d), must="conv2d_tune")[2]
            _, best, us = self._measure(self.lib.glsdet_conv2d_multi_tune, arr, n, must="conv2d_multi_tune")
            # grouped only where it is 5 % under the n launches, each tuned on its own, plus the credit for those it removes
            return best if us < 0.95 * single_us + (n - 1) * _fuse_credit_us() else -1

        hint = self._tune(key, measure)
        if hint < 0:
            return separate()
        return self.conv_multi(xs, packs, stride, pad, act, outs=outs, ress=ress, tile_hint=hint)

    def _shadow_begin(self, descs, outs, hint: int, multi: bool):
        """Run the conv(s) on kernel variant `hint` into dense scratch tensors BEFORE the real launch (an in-place
        conv still sees its original residual).  -> state for _shadow_end, or None if the variant declines."""
        n = len(descs)
        arr = (ConvDesc * n)()
        tmps = []
        for i, (d, o) in enumerate(zip(descs, outs)):
            C.memmove(C.addressof(arr[i]), C.addressof(d), C.sizeof(ConvDesc))
            t = self.tensor(o.n, o.h, o.w, o.c, o.dtype)
            tmps.append(t)
            arr[i].y = t.as_c()
            arr[i].tile_hint = hint
        st = _stream_ptr(self.stream)
        rc = self.lib.glsdet_conv2d_multi(arr, n, st) if multi else self.lib.glsdet_conv2d(C.byref(arr[0]), st)
        if rc != 0:                       # the variant does not take this problem
            return None
        return [(d.x.n, d.x.h, d.x.w, d.x.c, o.c, d.R, d.stride) for d, o in zip(descs, outs)], list(outs), tmps

    def _shadow_end(self, state):
        """After the real launch: element-wise distance of the variant's result from it."""
        if state is None:
            return
        for shape, o, t in zip(*state):
            self._shadow_record(shape, o, t, nan_in_ref=True)      # the variant under test is the `ref` side here

    def _shadow_record(self, shape, got: TView, ref: TView, nan_in_ref: bool = False):
        """One entry of shadow["log"]: how far `got` (the launch the plan keeps) is from `ref`, relative figures against got."""
        a, b = got.to_nchw(), ref.to_nchw()
        self.shadow["log"].append({"shape": shape, "scale": float(a.abs().max()), "err": float((a - b).abs().max()),
                                   "nan": bool(torch.isnan(b if nan_in_ref else a).any()), "differ": float((a != b).float().mean())})

    def pack_dw(self, w: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, c_pad: int):
        """depthwise weights [C,1,R,S] -> ([R*S][c_pad] in engine dtype, scale, bias, C, R, S)"""
        C_, one, R, S = w.shape
        assert one == 1 and C_ <= c_pad and c_pad % 8 == 0
        wp = torch.zeros(R * S, c_pad, dtype=torch.float32)
        wp[:, :C_] = w.float().reshape(C_, R * S).t()
        sc, bi = torch.ones(c_pad), torch.zeros(c_pad)
        sc[:C_], bi[:C_] = scale.float(), bias.float()
        return (self.upload(wp.to(_TORCH_DT[self.dt])), self.upload(sc), self.upload(bi), C_, R, S)

    def gate(self, a: TView, b: TView, gmap: Optional[TView], out: Optional[TView] = None) -> TView:
        """glsdet_gate: a * map[0] + b * map[1] with a map, a * b without"""
        if out is None:
            out = self.tensor(a.n, a.h, a.w, a.c, a.dtype)
        check(self.lib.glsdet_gate(C.byref(a.as_c()), C.byref(b.as_c()), C.byref(gmap.as_c()) if gmap is not None else None,
                                   C.byref(out.as_c()), 0 if gmap is not None else 1, _stream_ptr(self.stream)), "gate")
        return out

    def dwconv(self, x: TView, packed, stride: int, pad: int, act: str, out: Optional[TView] = None, dilation: int = 1) -> TView:
        R, S = packed[4:]
        ho = (x.h + 2 * pad - dilation * (R - 1) - 1) // stride + 1
        wo = (x.w + 2 * pad - dilation * (S - 1) - 1) // stride + 1
        if out is None:
            out = self.tensor(x.n, ho, wo, x.c, x.dtype)
        d = _conv_desc(x, packed, stride, pad, act, out)
        check(self.lib.glsdet_dwconv2d_dilated(C.byref(d), dilation, _stream_ptr(self.stream)), "dwconv2d")
        return out

    # ---- grouped 3x3 conv (ResNeXt conv2; glsdet_conv2d_grouped)
    def pack_conv_grouped(self, parts: Sequence[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]], groups: int) -> "GroupedPack":
        """parts: [(w [O, Cg, 3, 3] fp32, scale[O], bias[O])...] concatenated along O (O sums to groups * Cg).  Nothing is
        uploaded yet: the block layout of glsdet_conv2d_grouped (GroupedPack.blocks) and the block-diagonal dense pack
        (GroupedPack.dense: Engine.pack_conv over all C input channels) each when something first asks for it."""
        w = torch.cat([p[0].float() for p in parts], 0)
        scale = torch.cat([p[1].float() for p in parts], 0)
        bias = torch.cat([p[2].float() for p in parts], 0)
        return GroupedPack(self, w, scale, bias, groups)

    def conv_grouped(self, x: TView, packed: "GroupedPack", stride: int, act: str, out: Optional[TView] = None,
                     expand: Optional[bool] = None) -> TView:
        """act(scale * conv3x3_grouped(x) + bias), pad 1.  expand=True: as the block-diagonal dense conv through Engine.conv
        (C / Cg times the multiplies: the only form for a group width the kernel refuses, and the A/B partner of
        measurements); None: the grouped kernel where it takes the width -- under autotune only where it is not slower
        than the expansion on its tuned best variant (tuner key ("grouped", ...))."""
        assert x.c == packed.c, (x.c, packed.c)
        ho, wo = (x.h - 1) // stride + 1, (x.w - 1) // stride + 1
        if out is None:
            out = self.tensor(x.n, ho, wo, x.c, x.dtype)
        if expand is None:
            expand = not packed.kernel_takes
            if not expand and self.autotune:
                key = ("grouped",) + _in_geo(x) + _out_geo(out) + (packed.groups, stride, out.dtype)

                def measure():
                    d = _conv_desc(x, packed.blocks(), stride, 1, act, out)
                    rc, _, us = self._measure(self.lib.glsdet_conv2d_grouped_tune, C.byref(d), packed.groups)
                    if rc != 0:
                        return -1
                    dense = packed.dense(keep=False)            # held here until the tuner has run on it
                    dense_us = self._conv_us(_conv_desc(x, dense, stride, 1, act, out))
                    if dense_us is None or us <= dense_us:
                        return 0
                    packed.adopt(dense)                         # the expansion stays: the pack that was measured is the one kept
                    return -1

                expand = self._tune(key, measure) < 0
        if expand:
            return self.conv(x, packed.dense(), stride, 1, act, out=out)
        d = _conv_desc(x, packed.blocks(), stride, 1, act, out)
        check(self.lib.glsdet_conv2d_grouped(C.byref(d), packed.groups, _stream_ptr(self.stream)), "conv2d_grouped")
        if self.shadow is not None:             # against the block-diagonal expansion on the generic kernel
            ref = self.tensor(out.n, out.h, out.w, out.c, out.dtype)
            self.conv(x, packed.dense(), stride, 1, act, out=ref, tile_hint=1)
            self._shadow_record((x.n, out.h, out.w, x.c, x.c, 3, stride), out, ref)
        return out

    def focus_pack(self, img: torch.Tensor, out: Optional[TView] = None) -> TView:
        assert img.dtype == torch.float32 and img.is_contiguous() and img.device.type == "cuda"
        n, cin, H, W = img.shape
        if out is None:
            out = self.tensor(n, H // 2, W // 2, ceil_to(4 * cin, 8))
        check(self.lib.glsdet_focus_pack(img.data_ptr(), n, cin, H, W, C.byref(out.as_c()),
                                         _stream_ptr(self.stream)), "focus_pack")
        return out

    def focus_conv(self, img: torch.Tensor, packed, act: str, out: Optional[TView] = None) -> TView:
        """Focus + its 3x3 conv in one launch (glsdet_focus_conv); packed = pack_conv(..., cin_pad=16)."""
        assert img.dtype == torch.float32 and img.is_contiguous() and img.device.type == "cuda"
        n, cin, H, W = img.shape
        wdev, sdev, bdev, cout, R, S = packed
        assert (R, S) == (3, 3)
        if out is None:
            out = self.tensor(n, H // 2, W // 2, cout)
        check(self.lib.glsdet_focus_conv(img.data_ptr(), n, cin, H, W, wdev.data_ptr(), sdev.data_ptr(), bdev.data_ptr(),
                                         ACT[act], C.byref(out.as_c()), _stream_ptr(self.stream)), "focus_conv")
        return out

    def focus_conv_down(self, img: torch.Tensor, packed1, act1: str, packed2, act2: str, out: Optional[TView] = None) -> TView:
        """Focus + stem conv + the 3x3 stride-2 conv that follows, in one launch (glsdet_focus_conv_down)."""
        assert img.dtype == torch.float32 and img.is_contiguous() and img.device.type == "cuda"
        n, cin, H, W = img.shape
        w1, s1, b1, c1, R1, S1 = packed1
        w2, s2, b2, cout, R2, S2 = packed2
        assert (R1, S1, R2, S2) == (3, 3, 3, 3)
        if out is None:
            out = self.tensor(n, (H // 2 + 1) // 2, (W // 2 + 1) // 2, cout)
        check(self.lib.glsdet_focus_conv_down(img.data_ptr(), n, cin, H, W, w1.data_ptr(), s1.data_ptr(), b1.data_ptr(), ACT[act1], c1,
                                              w2.data_ptr(), s2.data_ptr(), b2.data_ptr(), ACT[act2], C.byref(out.as_c()),
                                              _stream_ptr(self.stream)), "focus_conv_down")
        return out

    def channel_maxmean(self, x: TView, out: Optional[TView] = None) -> TView:
        if out is None:
            out = self.tensor(x.n, x.h, x.w, 8, x.dtype)
        check(self.lib.glsdet_channel_maxmean(C.byref(x.as_c()), C.byref(out.as_c()), _stream_ptr(self.stream)),
              "channel_maxmean")
        return out

    def maxpool(self, x: TView, k: int, out: Optional[TView] = None) -> TView:
        if out is None:
            out = self.tensor(x.n, x.h, x.w, x.c, x.dtype)
        check(self.lib.glsdet_maxpool2d(C.byref(x.as_c()), C.byref(out.as_c()), k, _stream_ptr(self.stream)), "maxpool2d")
        return out

    def spp_pools(self, x: TView, y5: TView, y9: TView, y13: TView):
        check(self.lib.glsdet_spp_pools(C.byref(x.as_c()), C.byref(y5.as_c()), C.byref(y9.as_c()), C.byref(y13.as_c()),
                                        _stream_ptr(self.stream)), "spp_pools")

    def resample(self, x: TView, factor: int, out: Optional[TView] = None) -> TView:
        if out is None:
            out = self.tensor(x.n, x.h * factor, x.w * factor, x.c, x.dtype)
        check(self.lib.glsdet_resample_copy(C.byref(x.as_c()), C.byref(out.as_c()), factor,
                                            _stream_ptr(self.stream)), "resample_copy")
        return out

    def copy_many(self, xs: Sequence[TView], outs: Sequence[TView]) -> List[TView]:
        """xs[i] -> outs[i] (strided copies of equal extents, one dtype / channel count) in one launch per 32 pairs."""
        n = len(xs)
        assert n == len(outs) and n > 0
        xa = (View * n)(*[x.as_c() for x in xs])
        ya = (View * n)(*[y.as_c() for y in outs])
        check(self.lib.glsdet_copy_many(xa, ya, n, _stream_ptr(self.stream)), "copy_many")
        return list(outs)

    def transpose_many(self, xs: Sequence[TView], mats: Sequence[TView]) -> List[TView]:
        """mats[i][c][p] = xs[i] at pixel p, channel c (xs[i]: one image window, mats[i]: Engine.matrix with >= C rows and
        >= h*w columns): one launch per 32 pairs."""
        n = len(xs)
        assert n == len(mats) and n > 0
        xa = (View * n)(*[x.as_c() for x in xs])
        ya = (View * n)(*[y.as_c() for y in mats])
        check(self.lib.glsdet_transpose_many(xa, ya, n, _stream_ptr(self.stream)), "transpose_many")
        return list(mats)

    def nonlocal_(self, x: TView, tpg: TView, ci: int, wout: torch.Tensor, bout: torch.Tensor,
                  out: Optional[TView] = None) -> TView:
        if out is None:
            out = self.tensor(x.n, x.h, x.w, x.c, x.dtype)
        ws = self.raw(nonlocal_workspace_floats(1, x.n, ci, x.c) * 4)
        check(self.lib.glsdet_nonlocal(C.byref(x.as_c()), C.byref(tpg.as_c()), ci, wout.data_ptr(), bout.data_ptr(),
                                       ws.data_ptr(), C.byref(out.as_c()), _stream_ptr(self.stream)), "nonlocal")
        return out

    def nonlocal_mfma_takes(self, xs: Sequence[TView], tpgs: Sequence[TView], ci: int, outs: Sequence[TView], wouts=(), bouts=()) -> bool:
        """the preconditions of glsdet_nonlocal_mfma (include/glsdet_hip.h), evaluated without a call"""
        n = len(xs)
        if not 1 <= n <= 4 or len(tpgs) != n or len(outs) != n:
            return False
        cx, nimg, dt = xs[0].c, xs[0].n, xs[0].dtype
        if ci < 32 or ci % 32 or ci > 1280 or cx < 32 or cx % 32 or cx > 1280 or nimg * n > 65535:
            return False
        for x, t, o in zip(xs, tpgs, outs):
            if (x.c, x.n) != (cx, nimg) or (o.n, o.h, o.w, o.c) != (x.n, x.h, x.w, x.c) or (t.n, t.h, t.w) != (x.n, x.h, x.w):
                return False
            if t.c < 3 * ci or x.dtype != dt or t.dtype != dt or o.dtype != dt:
                return False
            vn = 16 // _ESIZE[dt]
            for v in (x, t, o):
                if v.off % vn or v.sn % vn or v.sh % vn or v.sw % vn or v.buf.data_ptr() % 16:
                    return False
        return all(w.data_ptr() % 16 == 0 for w in list(wouts) + list(bouts))

    # Where the matrix-core kernels beat the scalar ones beyond the scalar kernels' own run-to-run spread (DESIGN section 5:
    # tools/nonlocal_variants.py --sweep on an MI355X, batch 8, four quadrants, ci = cx): {width: smallest pixel count of the
    # largest set from which they won at every measured size}.  They won at every measured point, in both dtypes, so each
    # entry is the smallest quadrant that was measured; a width between two measured ones takes the larger of its
    # neighbours' entries, anything outside the measured range keeps the scalar kernels.
    NONLOCAL_MFMA_FROM = {c: 6 for c in (64, 96, 128, 192, 256, 320, 384, 512, 640, 1024, 1280)}

    def nonlocal_mfma_pays(self, xs: Sequence[TView], ci: int) -> bool:
        """the measured per-geometry choice behind mfma="auto"; GLSDET_NONLOCAL_MFMA=1 / 0 overrides it (measurements)"""
        forced = os.environ.get("GLSDET_NONLOCAL_MFMA", "")
        if forced in ("0", "1"):
            return forced == "1"
        t = self.NONLOCAL_MFMA_FROM
        if xs[0].c != ci or not min(t) <= ci <= max(t):
            return False
        need = max(t[max(c for c in t if c <= ci)], t[min(c for c in t if c >= ci)])
        return max(x.h * x.w for x in xs) >= need

    def nonlocal_multi(self, xs: Sequence[TView], tpgs: Sequence[TView], ci: int, wouts, bouts,
                       outs: Optional[Sequence[TView]] = None, mfma=False) -> List[TView]:
        """1..4 independent non-local blocks in one set of three launches, in place on each x unless `outs` is given.
        mfma=True: on the matrix-core kernels (glsdet_nonlocal_mfma) where they take the problem; "auto": where they take it
        AND were measured faster for the geometry (nonlocal_mfma_pays); the kernels of glsdet_nonlocal_multi otherwise --
        the default, so that every caller that does not ask keeps its bits.  A refusal of the entry point launches nothing
        and leads to the scalar kernels as well: the preconditions live in the library, nonlocal_mfma_takes only spares the
        call."""
        n = len(xs)
        outs = list(xs) if outs is None else list(outs)
        xa = (View * n)(*[x.as_c() for x in xs])
        oa = (View * n)(*[o.as_c() for o in outs])
        ta = (View * n)(*[t.as_c() for t in tpgs])
        wa = (C.c_void_p * n)(*[w.data_ptr() for w in wouts])
        ba = (C.c_void_p * n)(*[b.data_ptr() for b in bouts])
        if mfma and self.nonlocal_mfma_takes(xs, tpgs, ci, outs, wouts, bouts) and (mfma != "auto" or self.nonlocal_mfma_pays(xs, ci)):
            nbytes = self.lib.glsdet_nonlocal_mfma_workspace_bytes(xs[0].n, n, ci, xs[0].c)
            ws = self.raw(nbytes)
            if self.lib.glsdet_nonlocal_mfma(xa, ta, n, ci, wa, ba, ws.data_ptr(), nbytes, oa, _stream_ptr(self.stream)) == 0:
                return outs
        ws = self.raw(nonlocal_workspace_floats(n, xs[0].n, ci, xs[0].c) * 4)
        check(self.lib.glsdet_nonlocal_multi(xa, ta, n, ci, wa, ba, ws.data_ptr(), oa, _stream_ptr(self.stream)),
              "nonlocal_multi")
        return outs

    # ---- EVC block (csrc/evc.hip)
    def lvc_encode(self, x: TView, codewords: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
        """glsdet_lvc_encode: the codebook encoding of every image of x -> fp32 [n, 64, C]; codewords fp32 [64, C] and
        scale fp32 [64] on the device.  Workspace and result are allocated here, i.e. once, at plan build."""
        assert codewords.dtype == torch.float32 and tuple(codewords.shape) == (64, x.c) and scale.numel() == 64
        nbytes = self.lib.glsdet_lvc_encode_workspace_bytes(x.n, x.h, x.w, x.c)
        ws = self.raw(nbytes)
        E = self.raw(x.n * 64 * x.c * 4)[: x.n * 64 * x.c * 4].view(torch.float32).view(x.n, 64, x.c)
        check(self.lib.glsdet_lvc_encode(C.byref(x.as_c()), codewords.data_ptr(), scale.data_ptr(), ws.data_ptr(), nbytes,
                                         E.data_ptr(), _stream_ptr(self.stream)), "lvc_encode")
        return E

    def lvc_gate(self, E: torch.Tensor, n: int, c: int, a: torch.Tensor, b: torch.Tensor, fc_w: torch.Tensor,
                 fc_b: torch.Tensor) -> torch.Tensor:
        """glsdet_lvc_gate -> gam fp32 [n, C]"""
        assert tuple(E.shape) == (n, 64, c) and tuple(fc_w.shape) == (c, c) and a.numel() == 64 and b.numel() == 64
        gam = self.raw(n * c * 4)[: n * c * 4].view(torch.float32).view(n, c)
        check(self.lib.glsdet_lvc_gate(E.data_ptr(), n, c, a.data_ptr(), b.data_ptr(), fc_w.data_ptr(), fc_b.data_ptr(),
                                       gam.data_ptr(), _stream_ptr(self.stream)), "lvc_gate")
        return gam

    def channel_fuse(self, a: TView, t: Optional[TView], v: torch.Tensor, mode: int, out: Optional[TView] = None) -> TView:
        """glsdet_channel_fuse: mode 0 relu(a + a * v[n, c]), mode 1 a + v[c] * t"""
        if out is None:
            out = self.tensor(a.n, a.h, a.w, a.c, a.dtype)
        check(self.lib.glsdet_channel_fuse(C.byref(a.as_c()), C.byref(t.as_c()) if t is not None else None, C.byref(out.as_c()),
                                           v.data_ptr(), mode, _stream_ptr(self.stream)), "channel_fuse")
        return out

    # ---- Swin trunk (csrc/swin.hip)
    def layernorm(self, x: TView, gamma: torch.Tensor, beta: torch.Tensor, eps: float, out: Optional[TView] = None,
                  out_dtype: Optional[int] = None) -> TView:
        """glsdet_layernorm over the channels of every token; gamma / beta fp32 [C] on the device; the output may have
        another dtype than x (out_dtype, or out's)"""
        if out is None:
            out = self.tensor(x.n, x.h, x.w, x.c, x.dtype if out_dtype is None else out_dtype)
        assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == x.c == beta.numel()
        check(self.lib.glsdet_layernorm(C.byref(x.as_c()), C.byref(out.as_c()), gamma.data_ptr(), beta.data_ptr(), eps,
                                        _stream_ptr(self.stream)), "layernorm")
        return out

    def window_attention(self, qkv: TView, table: torch.Tensor, qkv_bias: Optional[torch.Tensor], heads: int, ws: int,
                         shift: int, scale: float, out: Optional[TView] = None) -> TView:
        """glsdet_window_attention: qkv [n, H, W, 3C] -> [n, H, W, C]; table fp32 [(2 ws - 1)^2, heads] and qkv_bias fp32
        [3C] (or None) on the device"""
        if out is None:
            out = self.tensor(qkv.n, qkv.h, qkv.w, qkv.c // 3, qkv.dtype)
        assert table.dtype == torch.float32 and tuple(table.shape) == ((2 * ws - 1) ** 2, heads)
        assert qkv_bias is None or (qkv_bias.dtype == torch.float32 and qkv_bias.numel() == qkv.c)
        check(self.lib.glsdet_window_attention(C.byref(qkv.as_c()), C.byref(out.as_c()), table.data_ptr(),
                                               qkv_bias.data_ptr() if qkv_bias is not None else None, heads, ws, shift,
                                               scale, _stream_ptr(self.stream)), "window_attention")
        return out

    def patch_merge(self, x: TView, out: Optional[TView] = None) -> TView:
        """glsdet_patch_merge: [n, H, W, C] -> [n, ceil(H / 2), ceil(W / 2), 4C] in nn.Unfold's channel order"""
        if out is None:
            out = self.tensor(x.n, (x.h + 1) // 2, (x.w + 1) // 2, 4 * x.c, x.dtype)
        check(self.lib.glsdet_patch_merge(C.byref(x.as_c()), C.byref(out.as_c()), _stream_ptr(self.stream)), "patch_merge")
        return out

    # ---- Patch_Conv_NonLocal_adapt_new: device-side quadrant split
    def attn_split(self, att: TView) -> torch.Tensor:
        """-> device int32[4] {row split, column split above it, column split from it on, 0} (glsdet_attn_split)."""
        split = torch.zeros(4, dtype=torch.int32, device=self.device)
        self._keep.append(split)
        check(self.lib.glsdet_attn_split(C.byref(att.as_c()), split.data_ptr(), _stream_ptr(self.stream)), "attn_split")
        return split

    def nonlocal_split(self, x: TView, tpgs: Sequence[TView], ci: int, wouts, bouts, out: TView, split: torch.Tensor,
                       shift: int = 0) -> TView:
        ws = self.raw(nonlocal_workspace_floats(4, x.n, ci, x.c) * 4)
        ta = (View * 4)(*[t.as_c() for t in tpgs])
        wa = (C.c_void_p * 4)(*[w.data_ptr() for w in wouts])
        ba = (C.c_void_p * 4)(*[b.data_ptr() for b in bouts])
        check(self.lib.glsdet_nonlocal_split(C.byref(x.as_c()), ta, ci, wa, ba, ws.data_ptr(), C.byref(out.as_c()),
                                             split.data_ptr(), shift, _stream_ptr(self.stream)), "nonlocal_split")
        return out

    def rowsplit(self, a: TView, b: Optional[TView], split: torch.Tensor, mode: int, out: Optional[TView] = None, quadrant: int = 0,
                 shift: int = 0) -> TView:
        """glsdet_rowsplit: 0 / 1 keep the rows above / from the split, 2 select a | b by row, 3 keep quadrant, 4 merge quadrant"""
        if out is None:
            out = self.tensor(a.n, a.h, a.w, a.c, a.dtype)
        check(self.lib.glsdet_rowsplit(C.byref(a.as_c()), C.byref(b.as_c()) if b is not None else None, C.byref(out.as_c()),
                                       split.data_ptr(), mode | (quadrant << 4) | (shift << 8), _stream_ptr(self.stream)), "rowsplit")
        return out

    def scale_by_map(self, x: TView, m: TView, out: Optional[TView] = None) -> TView:
        if out is None:
            out = self.tensor(x.n, x.h, x.w, x.c, x.dtype)
        check(self.lib.glsdet_scale_by_map(C.byref(x.as_c()), C.byref(m.as_c()), C.byref(out.as_c()), _stream_ptr(self.stream)),
              "scale_by_map")
        return out

    def decode(self, levels: Sequence[TView], num_classes: int, in_h: int, in_w: int,
               strides: Optional[Sequence[int]] = None, mode: int = 0, out: Optional[torch.Tensor] = None,
               scale_factors: Optional[torch.Tensor] = None, sigmoid: int = 3) -> torch.Tensor:
        """glsdet_yolox_decode_ex.  mode: box format (0 cx, cy, w, h / input size; 1 x1, y1, x2, y2 in pixels);
        sigmoid: bit 0 objectness, bit 1 classes -- channels outside the mask stay raw logits (DECODE_MODES)."""
        A = sum(l.h * l.w for l in levels)
        n = levels[0].n
        if out is None:
            out = torch.empty(n, A, 5 + num_classes, dtype=torch.float32, device=self.device)
            self._keep.append(out)
        arr = (View * len(levels))(*[l.as_c() for l in levels])
        st = (C.c_int32 * len(levels))(*strides) if strides is not None else None
        sf = None
        if scale_factors is not None:
            assert scale_factors.dtype == torch.float32 and scale_factors.is_contiguous() and scale_factors.numel() == 4 * n
            sf = scale_factors.data_ptr()
        check(self.lib.glsdet_yolox_decode_ex(arr, len(levels), num_classes, in_h, in_w, st, mode, int(sigmoid),
                                              out.data_ptr(), out.numel(), sf, _stream_ptr(self.stream)), "yolox_decode")
        return out

    def _result_buffers(self, ws_bytes: int, n: int, max_det: int, **extra):
        """What every NMS flavour writes into: the workspace, dets [n, max_det, 7], count [2n] (kept per image, then found
        per image) and the status word; `extra` = the sizes and inputs of the flavour."""
        return {"ws": self.raw(ws_bytes), "n": n, "max_det": max_det, **extra,
                "dets": torch.zeros(n, max_det, 7, dtype=torch.float32, device=self.device),
                "count": torch.zeros(2 * n, dtype=torch.int32, device=self.device),
                "status": torch.zeros(1, dtype=torch.int32, device=self.device)}

    def nms_buffers(self, n: int, A: int, max_cand: int, max_det: int):
        return self._result_buffers(self.lib.glsdet_nms_workspace_bytes(n, A, max_cand), n, max_det, A=A, max_cand=max_cand)

    def nms(self, pred: torch.Tensor, num_classes: int, box_mode: int, conf_thres: float, nms_thres: float, nb):
        n, A = pred.shape[0], pred.shape[1]
        assert pred.is_contiguous() and pred.dtype == torch.float32 and n == nb["n"] and A == nb["A"]
        check(self.lib.glsdet_nms(pred.data_ptr(), n, A, num_classes, box_mode, conf_thres, nms_thres,
                                  nb["max_cand"], nb["max_det"], nb["dets"].data_ptr(), nb["count"].data_ptr(),
                                  nb["status"].data_ptr(), nb["ws"].data_ptr(), nb["ws"].numel(),
                                  _stream_ptr(self.stream)), "nms")
        return nb["dets"], nb["count"], nb["status"]

    def pack_detections(self, nb, cap: int) -> torch.Tensor:
        """Append the fixed-capacity exchange record of the multi-GPU path to the op sequence:
        nb["packed"] = fp32 [n, cap+1, 7] (glsdet_pack_detections), allocated once here."""
        n = nb["dets"].shape[0]
        if "packed" not in nb or nb["packed"].shape[1] != cap + 1:
            nb["packed"] = torch.zeros(n, cap + 1, 7, dtype=torch.float32, device=self.device)
        check(self.lib.glsdet_pack_detections(nb["dets"].data_ptr(), nb["count"].data_ptr(), n, nb["max_det"], cap,
                                              nb["packed"].data_ptr(), _stream_ptr(self.stream)), "pack_detections")
        return nb["packed"]

    # ------------------------------------------------------------------ ResNet / FPN / GFL / MPHead ops
    def pack_resnet_stem(self, w: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor):
        """conv1.weight [64,3,7,7] -> [64][7][8][4] (tap 7 and channel 3 zero) in the engine dtype, + folded BN"""
        assert tuple(w.shape) == (64, 3, 7, 7)
        wp = torch.zeros(64, 7, 8, 4, dtype=torch.float32)
        wp[:, :, :7, :3] = w.float().permute(0, 2, 3, 1)
        assert wp.numel() == self.lib.glsdet_resnet_stem_weight_elems()
        return (self.upload(wp.to(_TORCH_DT[self.dt])), self.upload(scale.float()), self.upload(bias.float()))

    def resnet_stem(self, img: torch.Tensor, packed, act: str = "relu", out: Optional[TView] = None) -> TView:
        """7x7 stride-2 stem conv + BN + act straight from the fp32 NCHW image (glsdet_resnet_stem)"""
        assert img.dtype == torch.float32 and img.is_contiguous() and img.device.type == "cuda"
        n, cin, H, W = img.shape
        if out is None:
            out = self.tensor(n, (H + 1) // 2, (W + 1) // 2, 64)
        check(self.lib.glsdet_resnet_stem(img.data_ptr(), n, cin, H, W, packed[0].data_ptr(), packed[1].data_ptr(), packed[2].data_ptr(),
                                          ACT[act], C.byref(out.as_c()), _stream_ptr(self.stream)), "resnet_stem")
        return out

    def resnet_stem_pool(self, img: torch.Tensor, packed, out: Optional[TView] = None) -> TView:
        """... + ReLU + MaxPool2d(3, 2, 1) in the same launch (glsdet_resnet_stem_pool)"""
        assert img.dtype == torch.float32 and img.is_contiguous() and img.device.type == "cuda"
        n, cin, H, W = img.shape
        hc, wc = (H + 1) // 2, (W + 1) // 2
        if out is None:
            out = self.tensor(n, (hc + 1) // 2, (wc + 1) // 2, 64)
        check(self.lib.glsdet_resnet_stem_pool(img.data_ptr(), n, cin, H, W, packed[0].data_ptr(), packed[1].data_ptr(),
                                               packed[2].data_ptr(), C.byref(out.as_c()), _stream_ptr(self.stream)), "resnet_stem_pool")
        return out

    def nchw_pack(self, img: torch.Tensor, out: Optional[TView] = None) -> TView:
        assert img.dtype == torch.float32 and img.is_contiguous() and img.device.type == "cuda"
        n, cin, H, W = img.shape
        if out is None:
            out = self.tensor(n, H, W, ceil_to(cin, 8))
        check(self.lib.glsdet_nchw_pack(img.data_ptr(), n, cin, H, W, C.byref(out.as_c()), _stream_ptr(self.stream)),
              "nchw_pack")
        return out

    def pool2d(self, x: TView, k: int, stride: int, pad: int, out: Optional[TView] = None) -> TView:
        if out is None:
            out = self.tensor(x.n, (x.h + 2 * pad - k) // stride + 1, (x.w + 2 * pad - k) // stride + 1, x.c, x.dtype)
        check(self.lib.glsdet_pool2d(C.byref(x.as_c()), C.byref(out.as_c()), k, stride, pad, _stream_ptr(self.stream)),
              "pool2d")
        return out

    def upsample_add(self, coarse: TView, fine: TView) -> TView:
        check(self.lib.glsdet_upsample_add(C.byref(coarse.as_c()), C.byref(fine.as_c()), _stream_ptr(self.stream)),
              "upsample_add")
        return fine

    def groupnorm(self, x: TView, groups: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float, act: str = "relu",
                  out: Optional[TView] = None) -> TView:
        if out is None:
            out = x
        ws = self.raw(self.lib.glsdet_groupnorm_workspace_bytes(x.n, groups))
        check(self.lib.glsdet_groupnorm(C.byref(x.as_c()), C.byref(out.as_c()), groups, gamma.data_ptr(), beta.data_ptr(),
                                        eps, ACT[act], ws.data_ptr(), _stream_ptr(self.stream)), "groupnorm")
        return out

    def groupnorm_multi(self, xs: Sequence[TView], groups: int, gammas, betas, eps: float, act: str = "relu",
                        pre=None) -> List[TView]:
        """In place on each x: up to 16 tensors of the same n / C per launch pair.  pre[i]: the partial sums the conv
        that produced xs[i] already wrote (Engine.conv_gnstats), or None."""
        done = 0
        while done < len(xs):
            part = list(range(done, min(done + 16, len(xs))))
            n = len(part)
            ws = self.raw(n * self.lib.glsdet_groupnorm_workspace_bytes(xs[0].n, groups))
            xa = (View * n)(*[xs[i].as_c() for i in part])
            ga = (C.c_void_p * n)(*[gammas[i].data_ptr() for i in part])
            ba = (C.c_void_p * n)(*[betas[i].data_ptr() for i in part])
            if pre is not None and any(pre[i] is not None for i in part):
                pa = (C.c_void_p * n)(*[(pre[i].data_ptr() if pre[i] is not None else None) for i in part])
                check(self.lib.glsdet_groupnorm_multi_pre(xa, xa, n, groups, ga, ba, eps, ACT[act], ws.data_ptr(), pa,
                                                          _stream_ptr(self.stream)), "groupnorm_multi_pre")
            else:
                check(self.lib.glsdet_groupnorm_multi(xa, xa, n, groups, ga, ba, eps, ACT[act], ws.data_ptr(),
                                                      _stream_ptr(self.stream)), "groupnorm_multi")
            done += n
        return list(xs)

    def conv_gnstats(self, x: TView, packed, pad: int, groups: int, out: Optional[TView] = None):
        """3x3 stride-1 conv (no activation: GroupNorm follows) that also writes the GroupNorm partial sums of its output
        (glsdet_conv2d_gnstats).  -> (y, stats) or (y, None) when no statistics form applies or (autotune) the plain conv
        is faster by more than the statistics pass costs -- y is then produced by Engine.conv."""
        cout, R, S = packed[3:]
        if out is None:
            out = self.tensor(x.n, x.h + 2 * pad - R + 1, x.w + 2 * pad - S + 1, cout)
        # Off unless GLSDET_GN_FUSION=1: measured (MPDet, 8 x 800 x 1344, A/B on one box) the statistics pass it saves costs
        # 30 us per GroupNorm launch but the tower convs, MFMA bound at ~1000 TFLOP/s, pay 8 % for the sums in their store
        # phase (148 -> 162 us each): 1214 vs 1230 img/s.  The HBM-bound pass overlaps the other batches' convs; the convs do not.
        if (R, S, pad) != (3, 3, 1) or x.dtype != out.dtype or not os.environ.get("GLSDET_GN_FUSION"):
            return self.conv(x, packed, 1, pad, "none", out=out), None
        stats = self.raw(self.lib.glsdet_conv2d_gnstats_bytes(out.n, out.h, out.w, groups))
        d = _conv_desc(x, packed, 1, 1, "none", out, tile_hint=8)
        if self.autotune:
            def measure():
                rc, best, us = self._measure(self.lib.glsdet_conv2d_gnstats_tune, C.byref(d), groups, stats.data_ptr())
                if rc != 0:
                    return -1
                # against the plain conv's best variant + the statistics pass it saves (one read of the output at ~4 TB/s)
                d.tile_hint = 0
                u1 = self._conv_us(d)
                saved = out.n * out.h * out.w * out.c * _ESIZE[out.dtype] / 4e6
                return -1 if u1 is not None and us > u1 + saved else best

            d.tile_hint = self._tune(("gnstats",) + _in_geo(x) + _out_geo(out) + (groups, out.dtype), measure)
            if d.tile_hint < 0:
                return self.conv(x, packed, 1, pad, "none", out=out), None
        if self.lib.glsdet_conv2d_gnstats(C.byref(d), groups, stats.data_ptr(), _stream_ptr(self.stream)) != 0:
            return self.conv(x, packed, 1, pad, "none", out=out), None
        return out, stats

    def proxy_scores(self, feat: TView, dots: TView, counts: Sequence[int], gamma: float,
                     out: Optional[TView] = None) -> TView:
        nc = len(counts)
        if out is None:
            out = self.tensor(feat.n, feat.h, feat.w, ceil_to(nc, 8), F32)
        arr = (C.c_int32 * nc)(*counts)
        check(self.lib.glsdet_proxy_scores(C.byref(feat.as_c()), C.byref(dots.as_c()), arr, nc, gamma,
                                           C.byref(out.as_c()), _stream_ptr(self.stream)), "proxy_scores")
        return out

    def gfl_buffers(self, n: int, n_levels: int, max_cand: int, nms_pre: int, max_det: int):
        return self._result_buffers(self.lib.glsdet_gfl_workspace_bytes(n, n_levels, max_cand, nms_pre), n, max_det,
                                    max_cand=max_cand, nms_pre=nms_pre)

    @staticmethod
    def _gfl_levels(cls: Sequence[TView], reg: Sequence[TView], strides: Sequence[int], n: int,
                    img_hw: Optional[torch.Tensor], scale_factors: Optional[torch.Tensor] = None):
        """-> (cls views, reg views, strides, L) as the C arrays of glsdet_gfl_detect / glsdet_gfl_candidates; the optional
        per-image rows img_hw [n, 2] and scale_factors [n, 4] are checked here."""
        L = len(cls)
        for t, k in ((img_hw, 2), (scale_factors, 4)):
            assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == k * n)
        return ((View * L)(*[l.as_c() for l in cls]), (View * L)(*[l.as_c() for l in reg]), (C.c_int32 * L)(*strides), L)

    def gfl_detect(self, cls: Sequence[TView], reg: Sequence[TView], strides: Sequence[int], num_classes: int,
                   reg_max: int, in_h: int, in_w: int, score_thr: float, iou_thr: float, nb,
                   img_hw: Optional[torch.Tensor] = None, scale_factors: Optional[torch.Tensor] = None):
        ca, ra, st, L = self._gfl_levels(cls, reg, strides, nb["n"], img_hw, scale_factors)
        check(self.lib.glsdet_gfl_detect(ca, ra, L, st, num_classes, reg_max, in_h, in_w,
                                         img_hw.data_ptr() if img_hw is not None else None,
                                         scale_factors.data_ptr() if scale_factors is not None else None,
                                         score_thr, nb["nms_pre"], iou_thr, nb["max_cand"], nb["max_det"],
                                         nb["dets"].data_ptr(), nb["count"].data_ptr(), nb["status"].data_ptr(),
                                         nb["ws"].data_ptr(), nb["ws"].numel(), _stream_ptr(self.stream)), "gfl_detect")
        return nb["dets"], nb["count"], nb["status"]

    @staticmethod
    def gfl_candidate_cap(level_hw: Sequence[Tuple[int, int]], num_classes: int, nms_pre: int) -> int:
        """Rows per image of a candidate buffer: sum over the levels of min(nms_pre, H*W*nc)."""
        return sum(min(nms_pre, h * w * num_classes) for h, w in level_hw)

    def gfl_candidate_buffers(self, n: int, n_levels: int, max_cand: int, nms_pre: int, cap: int,
                              ws: Optional[torch.Tensor] = None):
        """Buffers of gfl_candidates.  Augmentations that share a plan share `ws` (their launches are ordered on one
        stream) and keep private `cand` / `cand_count`."""
        if ws is None:
            ws = self.raw(self.lib.glsdet_gfl_candidates_workspace_bytes(n, n_levels, max_cand))
        return {"ws": ws, "n": n, "max_cand": max_cand, "nms_pre": nms_pre, "cap": cap,
                "cand": torch.zeros(n, cap, 8, dtype=torch.float32, device=self.device),
                "cand_count": torch.zeros(n, dtype=torch.int32, device=self.device),
                "status": torch.zeros(1, dtype=torch.int32, device=self.device)}

    def gfl_candidates(self, cls: Sequence[TView], reg: Sequence[TView], strides: Sequence[int], num_classes: int,
                       reg_max: int, in_h: int, in_w: int, score_thr: float, cb, img_hw: Optional[torch.Tensor] = None):
        """glsdet_gfl_candidates: get_bboxes(..., rescale=False, with_nms=False) into cb (gfl_candidate_buffers)."""
        ca, ra, st, L = self._gfl_levels(cls, reg, strides, cb["n"], img_hw)
        check(self.lib.glsdet_gfl_candidates(ca, ra, L, st, num_classes, reg_max, in_h, in_w,
                                             img_hw.data_ptr() if img_hw is not None else None, score_thr,
                                             cb["nms_pre"], cb["max_cand"], cb["cand"].data_ptr(), cb["cap"],
                                             cb["cand_count"].data_ptr(), cb["status"].data_ptr(), cb["ws"].data_ptr(),
                                             cb["ws"].numel(), _stream_ptr(self.stream)), "gfl_candidates")
        return cb["cand"], cb["cand_count"], cb["status"]

    def aug_merge_buffers(self, n: int, caps: Sequence[int], max_det: int):
        K = len(caps)
        nbytes = self.lib.glsdet_aug_merge_workspace_bytes(n, (C.c_int32 * K)(*caps), K)
        if nbytes <= 0:
            raise _lib.GlsdetError("aug_merge_nms: %d augmentations with candidate capacities summing to %d; at most %d "
                              "augmentations and 32768 candidates per image (lower nms_pre)" % (K, sum(caps), 12))
        return self._result_buffers(nbytes, n, max_det, caps=tuple(caps),
                                    meta=torch.zeros(K, n, 8, dtype=torch.float32, device=self.device),
                                    out_scale=torch.ones(n, 4, dtype=torch.float32, device=self.device))

    def aug_merge_nms(self, cands: Sequence[torch.Tensor], counts: Sequence[torch.Tensor], iou_thr: float, mb,
                      use_out_scale: bool = False):
        """glsdet_aug_merge_nms over K candidate lists ([n, cap_k, 8] fp32 + int32 [n] counts); the per-augmentation
        meta rows and the output scale are read from mb["meta"] / mb["out_scale"] when the launch runs."""
        K, n = len(cands), mb["n"]
        assert K == len(counts) == len(mb["caps"])
        for t, c, cap in zip(cands, counts, mb["caps"]):
            assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (n, cap, 8)
            assert c.dtype == torch.int32 and c.is_contiguous() and c.numel() == n
        pa = (C.c_void_p * K)(*[t.data_ptr() for t in cands])
        pc = (C.c_void_p * K)(*[t.data_ptr() for t in counts])
        check(self.lib.glsdet_aug_merge_nms(pa, pc, (C.c_int32 * K)(*mb["caps"]), K, n, mb["meta"].data_ptr(), iou_thr,
                                            mb["max_det"], mb["out_scale"].data_ptr() if use_out_scale else None,
                                            mb["dets"].data_ptr(), mb["count"].data_ptr(), mb["status"].data_ptr(),
                                            mb["ws"].data_ptr(), mb["ws"].numel(), _stream_ptr(self.stream)),
              "aug_merge_nms")
        return mb["dets"], mb["count"], mb["status"]

    SOFT_NMS_METHODS = {"linear": 1, "gaussian": 2, "hard": 3}

    def soft_nms_buffers(self, n: int, cap: int, max_det: int):
        nbytes = self.lib.glsdet_soft_nms_workspace_bytes(n, cap)
        if nbytes <= 0 or max_det < 1:
            raise _lib.GlsdetError("soft_nms: n %d, cap %d, max_det %d; need n >= 1, 1 <= cap <= 32768, max_det >= 1"
                                   % (n, cap, max_det))
        return self._result_buffers(nbytes, n, max_det, cap=cap, segment_limit=int(self.lib.glsdet_soft_nms_segment_limit()))

    def soft_nms(self, cand: torch.Tensor, counts: torch.Tensor, num_classes: int, sb, method: str = "gaussian",
                 iou_thr: float = 0.3, sigma: float = 0.5, min_score: float = 1e-4, rescore: bool = False):
        """glsdet_soft_nms (drone/merge_results.py:41-130) over candidate rows [n, cap, 8] fp32 + int32 [n] counts into sb
        (soft_nms_buffers): dets rows x1,y1,x2,y2, original score, decayed score, label in descending original score
        (rescore: decayed score).  status bit0: a count above cap, bit1: a class segment above sb["segment_limit"] or a
        label outside [0, num_classes) -- the caller raises on either."""
        if method not in self.SOFT_NMS_METHODS:
            raise ValueError("soft_nms: method %r is not one of %s" % (method, sorted(self.SOFT_NMS_METHODS)))
        n, cap = sb["n"], sb["cap"]
        assert cand.dtype == torch.float32 and cand.is_contiguous() and tuple(cand.shape) == (n, cap, 8)
        assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == n
        check(self.lib.glsdet_soft_nms(cand.data_ptr(), counts.data_ptr(), n, cap, num_classes, self.SOFT_NMS_METHODS[method],
                                       iou_thr, sigma, min_score, int(bool(rescore)), sb["max_det"], sb["dets"].data_ptr(),
                                       sb["count"].data_ptr(), sb["status"].data_ptr(), sb["ws"].data_ptr(), sb["ws"].numel(),
                                       _stream_ptr(self.stream)), "soft_nms")
        return sb["dets"], sb["count"], sb["status"]

    def branch(self, b: int):
        """Ops emitted until the next branch(0) belong to independent branch b (1..8): quadrant
        convs, the l/r/t/b stitch convs, the cls/reg towers.  No-op outside plan recording."""
        # Opt-in (GLSDET_BRANCHES=1).  Measured on MI355X: alone, forking the quadrant / tower
        # convs into parallel graph branches gains ~2 %; with two batches in flight (bench) the
        # fork/join nodes serialise the two graphs against each other and cost 15 % img/s.
        if not os.environ.get("GLSDET_BRANCHES"):
            return
        check(self.lib.glsdet_plan_set_branch(b), "plan_set_branch")

    def save_tune_cache(self):
        if not self._tune_cache_path or not self._tune_dirty:
            return
        with _TUNE_IO_LOCK:                         # other lanes' tuners insert into the shared table meanwhile: snapshot it
            data = {}
            if os.path.exists(self._tune_cache_path):
                try:
                    with open(self._tune_cache_path) as f:
                        data = json.load(f)
                except ValueError:                  # another rank's half-written file from before the rename below existed
                    data = {}
            data[self._dtype_name] = {json.dumps(list(k)): v for k, v in list(self._tuned.items())}
            tmp = "%s.%d.%d.tmp" % (self._tune_cache_path, os.getpid(), threading.get_ident())   # whole files only, one tmp per writer
            with open(tmp, "w") as f:
                json.dump(data, f)
            os.replace(tmp, self._tune_cache_path)
            self._tune_dirty = False

    def new_plan(self) -> Plan:
        return Plan(self.lib)


def _fuse_credit_us() -> float:
    """Experiment switch (GLSDET_FUSE_CREDIT_US, default 0): microseconds a fused form is credited per launch it removes when
    the tuner compares it with the separate launches (the graph edge a removed launch no longer pays is not in either timing)."""
    return float(os.environ.get("GLSDET_FUSE_CREDIT_US", "0"))


def fold_bn(gamma, beta, mean, var, eps: float):
    """BatchNorm (eval) -> per-channel scale/bias, computed in fp64."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    return s.float(), (beta.double() - mean.double() * s).float()
