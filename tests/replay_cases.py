"""One small case per launching entry point of the C ABI, for the replay-invariance tests.

Production records ops into a glsdet_plan once and replays the plan, eagerly or from a captured hipGraph, for every frame
into the same buffers.  A case here is one such call through the raw C ABI:

  record(lib, stream)   makes the call with ctypes objects built for this call (inside a recording it appends an op,
                        outside it launches); every ctypes object that reaches the library is noted
  destroy_host_args()   overwrites those objects with 0xA5 bytes and drops them: what the closure did not copy is gone
  load(k)               writes data set k in place into the fixed device buffers
  outputs()             every output buffer, whole (margins, status and count words included), as bytes
  dirty(ws)             0xFF bytes into the outputs (and the workspaces)
  inputs_changed(k)     names of the input buffers that no longer hold data set k
  check_want(k, outs)   differences from the family's bit-exact reference (tests/*_reference.py), where it has one

Buffers are bound either to fabricated addresses (CPU tests: recording never dereferences them) or to one device
allocation per case (GPU tests)."""
import collections
import ctypes as C
import fnmatch
import zlib

import numpy as np

EXCLUDED = ("*_tune", "*_bytes", "*_elems", "glsdet_plan_*", "glsdet_abi_version", "glsdet_last_error", "glsdet_conv_kpad",
            "glsdet_conv_cout_pad", "glsdet_jpeg_parse", "glsdet_jpeg_entropy_decode", "glsdet_soft_nms_segment_limit",
            "glsdet_ufp_pack_max_boxes")
FAKE = 0x40000000                       # fabricated addresses: FAKE + i * 64 MiB, 256-byte aligned
F16, F32 = 0, 1
NP = {F16: np.float16, F32: np.float32}


def required_exports():
    from glsdet_amd import _lib
    return sorted(n for n in _lib._SIGS if not any(fnmatch.fnmatchcase(n, p) for p in EXCLUDED))


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def rnd(dtype, nbytes, *key):
    """nbytes of small exact values (eighths in [-2, 2]) of `dtype`, a function of the key alone"""
    dtype = np.dtype(dtype)
    n = -(-nbytes // dtype.itemsize)
    v = np.random.default_rng(_seed(*key)).integers(-16, 17, n)
    v = (v / 8.0).astype(dtype) if dtype.kind == "f" else (v + 16).astype(dtype)
    return v.view(np.uint8)[:nbytes]


def raw(a, nbytes=None):
    """an array's bytes, zero padded to nbytes"""
    b = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    if nbytes is None or b.size == nbytes:
        return b
    assert b.size <= nbytes, (b.size, nbytes)
    out = np.zeros(nbytes, np.uint8)
    out[: b.size] = b
    return out


class Spy:
    """the library with every ctypes object that is passed to it noted in `kept`"""

    def __init__(self, lib, kept):
        self._lib, self._kept = lib, kept

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            for a in args:
                obj = getattr(a, "_obj", a)             # byref(x) -> x
                if isinstance(obj, (C.Structure, C.Array)):
                    self._kept.append(obj)
            return fn(*args)
        return call


class Buf:
    def __init__(self, name, nbytes, role, data):
        self.name, self.nbytes, self.role, self.data, self.off = name, int(nbytes), role, data, None


class Case:
    """call(lib, case, stream) -> rc makes the one call; buffers are declared with buf() before binding"""

    def __init__(self, key, export, call, n_sets=2, in_place=False, want=None, note=""):
        self.key, self.export, self.call, self.n_sets, self.in_place, self._want, self.note = key, export, call, n_sets, in_place, want, note
        self.bufs = collections.OrderedDict()
        self.base, self.mem, self.kept = None, None, []

    # ---- declaration
    def buf(self, name, nbytes, role, data=None):
        """role: "in" (data(k) -> bytes), "out", "ws", "inout" (loaded like an input, compared like an output)"""
        assert role in ("in", "out", "ws", "inout") and name not in self.bufs and nbytes > 0
        assert (data is not None) == (role in ("in", "inout")), name
        self.bufs[name] = Buf(name, nbytes, role, data)
        return self

    def _layout(self):
        off = 0
        for b in self.bufs.values():
            b.off = off
            off += (b.nbytes + 255) // 256 * 256 + 256
        return off

    def bind_fake(self, index):
        assert self._layout() <= 64 << 20
        self.base, self.mem = FAKE + index * (64 << 20), None
        return self

    def bind_device(self):
        import torch
        self.mem = torch.empty(self._layout(), dtype=torch.uint8, device="cuda:0")
        self.mem.fill_(0xFF)
        self.base = self.mem.data_ptr()
        assert self.base % 256 == 0
        return self

    # ---- what a call uses
    def addr(self, name):
        return self.base + self.bufs[name].off

    def nbytes(self, name):
        return self.bufs[name].nbytes

    def view(self, name, n, h, w, c, dt, ct=0, off=0):
        """a dense NHWC view (pixel stride ct or c) `off` elements into buffer `name`, which is its allocation"""
        from glsdet_amd import _lib
        es = 2 if dt == F16 else 4
        ct = ct or c
        v = _lib.View()
        v.base, v.n, v.h, v.w, v.c, v.dtype = self.addr(name) + off * es, n, h, w, c, dt
        v.sw, v.sh, v.sn = ct, w * ct, h * w * ct
        v.alloc_lo, v.alloc_hi = self.addr(name), self.addr(name) + self.nbytes(name)
        assert v.base + ((n - 1) * v.sn + (h - 1) * v.sh + (w - 1) * v.sw + c) * es <= v.alloc_hi, name
        return v

    # ---- the protocol
    def record(self, lib, stream=None):
        rc = self.call(Spy(lib, self.kept), self, stream)
        assert rc == 0, "%s: rc %d: %s" % (self.key, rc, lib.glsdet_last_error().decode(errors="replace"))

    def destroy_host_args(self):
        n = len(self.kept)
        for obj in self.kept:
            C.memset(C.addressof(obj), 0xA5, C.sizeof(obj))
        del self.kept[:]
        return n

    def _dev(self, b):
        return self.mem[b.off: b.off + b.nbytes]

    def load(self, k):
        import torch
        for b in self.bufs.values():
            if b.role in ("in", "inout"):
                self._dev(b).copy_(torch.from_numpy(np.array(self.host(b.name, k))))

    def host(self, name, k):
        b = self.bufs[name]
        return raw(b.data(k), b.nbytes)

    def outputs(self):
        import torch
        torch.cuda.synchronize()
        return collections.OrderedDict((b.name, self._dev(b).cpu().numpy().copy()) for b in self.bufs.values() if b.role in ("out", "inout"))

    def dirty(self, ws=True):
        for b in self.bufs.values():
            if b.role == "out" or (ws and b.role == "ws"):
                self._dev(b).fill_(0xFF)

    def inputs_changed(self, k):
        import torch
        torch.cuda.synchronize()
        return [b.name for b in self.bufs.values() if b.role == "in" and not np.array_equal(self._dev(b).cpu().numpy(), self.host(b.name, k))]

    @property
    def has_want(self):
        return self._want is not None

    def check_want(self, k, outs):
        """-> messages: where `outs` (of outputs()) differs from the reference of data set k"""
        return self._want(k, outs)


def differing(got, ref):
    """names of the output buffers whose bytes differ, with the first differing byte"""
    out = []
    for name in ref:
        if not np.array_equal(got[name], ref[name]):
            at = int(np.nonzero(got[name] != ref[name])[0][0])
            out.append("%s: %d bytes differ, the first at %d (got %#x, want %#x)" % (name, int((got[name] != ref[name]).sum()), at, got[name][at], ref[name][at]))
    return out


# ====================================================================================================== the helper entry points
# tests/test_helper_host_cpu.py's Entry list: its accepted call per entry point, with the fabricated slots P + (slot << 20)
# bound to buffers of the case.  key -> role of the operand's slot; every other slot is an input.
HELPER_ROLES = {
    "focus_pack": {"y": "out"}, "maxpool2d": {"y": "out"}, "spp_pools": {"y5": "out", "y9": "out", "y13": "out"},
    "channel_maxmean": {"y": "out"}, "resample_copy": {"y": "out"}, "copy_many": {"y": "out"}, "transpose_many": {"y": "out"},
    "attn_split": {"split": "out"}, "rowsplit": {"y": "inout"}, "scale_by_map": {"y": "out"}, "gate": {"y": "out"},
    "nchw_pack": {"y": "out"}, "pool2d": {"y": "out"}, "upsample_add": {"fine": "inout"},
    "groupnorm": {"y": "out", "stats": "ws"}, "groupnorm_multi": {"y": "out", "stats": "ws"},
    "groupnorm_multi_pre": {"y": "out", "stats": "ws"}, "proxy_scores": {"out": "out"},
    "lvc_encode": {"E": "out", "ws": "ws"}, "lvc_gate": {"gam": "out"}, "channel_fuse": {"y": "out"}, "layernorm": {"y": "out"},
    "patch_merge": {"y": "out"}, "window_attention": {"y": "out"}, "dwconv2d_dilated": {"d.y": "out"},
    "focus_conv": {"y": "out"}, "focus_conv_down": {"y": "out"}, "resnet_stem": {"y": "out"}, "resnet_stem_pool": {"y": "out"},
}
IN_PLACE = {"rowsplit", "upsample_add"}                 # y keeps what the op does not write / fine is read and written
RAW_BYTES = 256 << 10                                   # a pointer operand that is no view: its buffer
ROW_SPLITS = [(3, 4, 5), (2, 3, 6), (4, 6, 2)]          # (row, column above, column below) on the 6 x 8 map of the rowsplit entry


def _refs(a):
    """(key, view) and (key, (container, index or attribute)) of every device address in an Entry's argument dict"""
    from glsdet_amd import _lib
    from tests.test_helper_host_cpu import P
    for k, v in a.items():
        if isinstance(v, _lib.View):
            yield k, v
        elif isinstance(v, _lib.ConvDesc):
            for m in ("x", "y", "res"):
                if getattr(v, m).base:
                    yield k + "." + m, getattr(v, m)
            for m in ("w", "scale", "bias"):
                yield k + "." + m, (v, m)
        elif isinstance(v, list):
            for i, q in enumerate(v):
                if isinstance(q, _lib.View):
                    yield k, q
                elif isinstance(q, int) and not isinstance(q, bool) and q >= P:
                    yield k, (v, i)
        elif isinstance(v, int) and not isinstance(v, bool) and v >= P:
            yield k, (a, k)


def _get(ref):
    box, i = ref
    return getattr(box, i) if isinstance(i, str) and not isinstance(box, dict) else box[i]


def _set(ref, value):
    box, i = ref
    if isinstance(i, str) and not isinstance(box, dict):
        setattr(box, i, value)
    else:
        box[i] = value


def _helper_case(e, dt):
    from glsdet_amd import _lib
    from tests.test_helper_host_cpu import P
    roles = HELPER_ROLES[e.name]
    a0 = dict(e.args(dt), dt=dt)
    slots = collections.OrderedDict()                   # slot -> [bytes, numpy dtype, role, key]
    for key, ref in _refs(a0):
        if isinstance(ref, _lib.View):
            slot, size, npdt = (ref.alloc_lo - P) >> 20, ref.alloc_hi - ref.alloc_lo, NP[ref.dtype]
        else:
            slot, size = (_get(ref) - P) >> 20, RAW_BYTES
            npdt = NP[dt] if key.split(".")[-1] in ("w", "w2") else np.int32 if key == "split" else np.float32
        size = a0["ws_bytes"] if key == "ws" else size
        s = slots.setdefault(slot, [0, npdt, "in", key])
        s[0] = max(s[0], size)
        if key in roles:
            s[2] = roles[key]
    assert {s[3] for s in slots.values() if s[2] != "in"} == set(roles), (e.name, roles)

    def call(lib, case, st):
        from tests import test_helper_host_cpu as H
        a = dict(e.args(dt), dt=dt)
        for key, ref in _refs(a):
            if isinstance(ref, _lib.View):
                slot = (ref.alloc_lo - P) >> 20
                delta = case.addr("s%d" % slot) - (P + (slot << 20))
                ref.base, ref.alloc_lo, ref.alloc_hi = ref.base + delta, ref.alloc_lo + delta, ref.alloc_hi + delta
            else:
                slot = (_get(ref) - P) >> 20
                _set(ref, _get(ref) + case.addr("s%d" % slot) - (P + (slot << 20)))
        entry = [q for q in H._entries(_Streamed(lib, st)) if q.name == e.name][0]
        return entry.call(a)

    case = Case(e.name, "glsdet_" + e.name, call, n_sets=3 if e.name == "rowsplit" else 2, in_place=e.name in IN_PLACE,
                note=NO_WANT.get(e.name, ""))
    if e.name in _helper_wants():
        case._want = _helper_want(e, dt, case, _helper_wants()[e.name])
    else:
        assert e.name in NO_WANT, e.name
    for slot, (size, npdt, role, key) in slots.items():
        name = "s%d" % slot
        if key == "split" and role == "in":
            data = lambda k: np.array(ROW_SPLITS[k] + (0,), np.int32)
        elif e.name == "attn_split" and role == "in":
            data = lambda k, npdt=npdt, size=size: _attention_map(k, npdt, size)
        else:
            data = None if role in ("out", "ws") else (lambda k, npdt=npdt, size=size, name=name: rnd(npdt, size, e.name, name, k))
        case.buf(name, size, role, data)
    return case


def _attention_map(k, npdt, nbytes):
    """2 x 16 x 16 x 1: a low floor and one bright 5 x 5 block per image whose place depends on the data set: the centroid
    walk of glsdet_attn_split ends elsewhere"""
    m = np.full((2, 16, 16), 0.125, np.float64)
    y, x = ((2, 3), (9, 10))[k]
    m[:, y: y + 5, x: x + 5] = 1.0 + np.arange(25).reshape(5, 5) / 32.0
    return raw(m.astype(npdt), nbytes)


# ---- bit-exact references of the helper cases.  The generic data (eighths in [-2, 2]) lies in the exact regime of these
# operations: a maximum, a copy or one conversion of such a value is exact in fp16 and fp32, a sum of two and a product of
# two plus a third (64ths below 6) likewise.  fn(a, x, dt) -> {output key: NCHW float64 array, or a list of them}; a = the
# Entry's argument dict, x = {input key: NCHW float64 array(s) as loaded}, dt = "f16" / "f32".
def _helper_wants():
    from tests import helper_reference as HR
    upcat = lambda a, x, dt: {"fine": HR.upsample_add_ref(x["fine"], x["coarse"], dt)}
    return {
        "maxpool2d": lambda a, x, dt: {"y": HR.maxpool_ref(x["x"], a["k"])},
        "pool2d": lambda a, x, dt: {"y": HR.pool2d_ref(x["x"], a["k"], a["stride"], a["pad"])},
        "spp_pools": lambda a, x, dt: dict(zip(("y5", "y9", "y13"), HR.spp_ref(x["x"]))),
        "resample_copy": lambda a, x, dt: {"y": HR.resample_ref(x["x"], a["factor"])},
        "copy_many": lambda a, x, dt: {"y": [HR.copy_ref(q) for q in x["x"]]},
        "focus_pack": lambda a, x, dt: {"y": HR.focus_ref(x["img"], a["y"].c, dt)},
        "nchw_pack": lambda a, x, dt: {"y": HR.nchw_pack_ref(x["img"], a["y"].c, dt)},
        "upsample_add": upcat,
        "scale_by_map": lambda a, x, dt: {"y": HR.stored(x["x"] * x["map"][:, :1], dt)},
        "gate": lambda a, x, dt: {"y": HR.stored(x["a"] * x["map"][:, 0:1] + x["b"] * x["map"][:, 1:2], dt)},        # mode 0: the map weighs a and b
        "rowsplit": lambda a, x, dt: {"y": np.where((np.arange(x["a"].shape[2]) < x["split"][0])[None, None, :, None], x["a"], x["b"])},
        "attn_split": _attn_split_want,
        "patch_merge": _patch_merge_want,
        "channel_maxmean": _maxmean_want,
        "transpose_many": lambda a, x, dt: {"y": [_transposed(q, v, dt) for q, v in zip(x["x"], a["y"])]},
        "channel_fuse": lambda a, x, dt: {"y": HR.stored(x["a"] + x["v"].reshape(-1)[None, : x["a"].shape[1], None, None] * x["t"], dt)},
    }


def _attn_split_want(a, x, dt):
    """tests/attention_reference.split_reference on the map in units of 1/32 (the map of _attention_map is exact in them)"""
    from tests import attention_reference as AR
    m = x["att"][:, 0] * 32.0
    assert np.array_equal(m, np.round(m))
    return {"split": np.array(AR.split_reference(m.astype(np.int64)) + (0,), np.int32)}


def _patch_merge_want(a, x, dt):
    import torch
    from tests import swin_reference as S
    y = S.patch_merge(torch.from_numpy(np.ascontiguousarray(x["x"].transpose(0, 2, 3, 1))))
    return {"y": y.numpy().transpose(0, 3, 1, 2)}


def _maxmean_want(a, x, dt):
    """channel 0 the maximum, channel 1 the mean, the rest zero.  32 channels of eighths: the sum is exact in fp32 and the
    division by 32 a power of two, so the mean is exact in either dtype whatever the order of the additions"""
    from tests import helper_reference as HR
    v = x["x"]
    assert v.shape[1] & (v.shape[1] - 1) == 0
    y = np.zeros((v.shape[0], a["y"].c) + v.shape[2:])
    y[:, 0], y[:, 1] = v.max(1), v.sum(1) / v.shape[1]
    return {"y": HR.stored(y, dt)}


def _transposed(x, v, dt):
    """tests/helper_reference.transpose_dest_ref for a destination matrix [v.w rows][v.c columns] whose columns all lie below
    ceil_vec(pixels): nothing of its prior contents survives, so `before` is immaterial"""
    from tests import helper_reference as HR
    assert HR.ceil_to(x.shape[2] * x.shape[3], HR.VN[dt]) == v.c and x.shape[1] == v.w
    m = HR.transpose_dest_ref(x, v.w, v.c, HR.VN[dt], np.zeros((v.w, v.c)))
    return m.T[None, :, None, :]


# why a helper case has no reference of its own (it is then held to the immediate launch alone)
NO_WANT = {
    "groupnorm": "bit-exact only on helper_reference.gn_exact_data; generic data is held to the bound B, not bit for bit",
    "groupnorm_multi": "as groupnorm", "groupnorm_multi_pre": "as groupnorm; the conv partial sums are generic too",
    "proxy_scores": "held to PROXY_TOL, not bit for bit", "lvc_encode": "bit-exact only on cfp_reference's 'uniform' operands",
    "lvc_gate": "expf: held to a bound", "layernorm": "bit-exact only on test_swin_exact._two_value data",
    "window_attention": "bit-exact only on the one-hot operands of swin_reference",
    "dwconv2d_dilated": "SiLU epilogue: held at ulp level (tests/test_act_exact.py), not bit for bit",
    "focus_conv": "as dwconv2d_dilated", "focus_conv_down": "as dwconv2d_dilated", "resnet_stem": "as dwconv2d_dilated",
    "resnet_stem_pool": "as dwconv2d_dilated",
}


def _nchw(bytes_, v, npdt):
    """the elements of the dense view v (at the start of its buffer) as float64 NCHW"""
    ct = v.sw
    a = bytes_[: v.n * v.h * v.w * ct * np.dtype(npdt).itemsize].view(npdt).reshape(v.n, v.h, v.w, ct)[..., : v.c]
    return a.astype(np.float64).transpose(0, 3, 1, 2)


def _helper_want(e, dt, case, fn):
    """want(k, outs) of a helper case from fn (see _helper_wants): the view's elements bit for bit (+0.0 and -0.0 apart), and
    every byte of the output buffer outside the view still 0xFF"""
    from glsdet_amd import _lib
    from tests.test_helper_host_cpu import P
    a0 = dict(e.args(dt), dt=dt)
    slot = lambda ref: "s%d" % (((ref.alloc_lo if isinstance(ref, _lib.View) else _get(ref)) - P) >> 20)
    refs = collections.OrderedDict()
    for key, ref in _refs(a0):
        refs.setdefault(key, []).append(ref)
    name = "f16" if dt == F16 else "f32"

    def want(k, outs):
        x = {}
        for key, rs in refs.items():
            if case.bufs[slot(rs[0])].role in ("out", "ws"):
                continue
            vals = [_nchw(case.host(slot(r), k), r, NP[r.dtype]) if isinstance(r, _lib.View) else None for r in rs]
            if vals[0] is None:                          # a plain array: fp32, in the layout the entry point documents
                b = case.host(slot(rs[0]), k).view(np.float32).astype(np.float64)
                vals = [b[: a0["n"] * a0["cin"] * a0["H"] * a0["W"]].reshape(a0["n"], a0["cin"], a0["H"], a0["W"])] if key == "img" else [b]
                if key == "split":
                    vals = [case.host(slot(rs[0]), k).view(np.int32)[:4]]
            x[key] = vals if isinstance(a0[key], list) else vals[0]
        bad = []
        for key, w in fn(a0, x, name).items():
            for r, wq in zip(refs[key], w if isinstance(w, list) else [w]):
                if not isinstance(r, _lib.View):         # a plain array: the reference's bytes, then nothing written
                    full = np.full(outs[slot(r)].size, 0xFF, np.uint8)
                    full[: wq.nbytes] = raw(wq)
                    bad += _cmp("%s (%s)" % (key, slot(r)), outs[slot(r)], full)
                    continue
                got, npdt = outs[slot(r)], NP[r.dtype]
                full = np.full(got.size, 0xFF, np.uint8) if case.bufs[slot(r)].role == "out" else case.host(slot(r), k).copy()
                nel = r.n * r.h * r.w * r.sw
                img = full[: nel * np.dtype(npdt).itemsize].view(npdt).reshape(r.n, r.h, r.w, r.sw)
                img[..., : r.c] = np.asarray(wq, np.float64).transpose(0, 2, 3, 1).astype(npdt)
                bad += _cmp("%s (%s)" % (key, slot(r)), got, full)
        return bad
    return want


class _Streamed:
    """the Entry table passes a null stream: put the case's stream in its place (the last argument of every entry point)"""

    def __init__(self, lib, st):
        self._lib, self._st = lib, st

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.endswith("_bytes"):
            return fn
        return lambda *args: fn(*(args[:-1] + (self._st,)))


def _helper_cases():
    from tests import test_helper_host_cpu as H
    from glsdet_amd import _lib
    return [_helper_case(e, e.dtypes[0]) for e in H._entries(_lib.load())]


# ============================================================================================================ the conv family
# Generic data (eighths in [-2, 2]) in x, the packed weights, scale and bias: every byte pattern is a weight, and the replay
# must reproduce the immediate launch whatever the values are.  fp16, the production dtype.
def _binding():
    from glsdet_amd import _lib
    return _lib, _lib.load()


def _gen(case, name, nbytes, dtype=np.float16, role="in"):
    return case.buf(name, nbytes, role, (lambda k: rnd(dtype, nbytes, case.key, name, k)) if role in ("in", "inout") else None)


def _conv_bufs(case, names, x=(2, 9, 11, 64)):
    """x-like fp16 buffers for every name in `names` (role by prefix: x in, everything else out), weights by the caller"""
    n, h, w, c = x
    for nm in names:
        _gen(case, nm, n * h * w * c * 2, np.float16, "in" if nm.startswith("x") else "out")


def _wsb(case, tag, wbytes=RAW_BYTES):
    _gen(case, "w" + tag, wbytes, np.float16)
    _gen(case, "scale" + tag, 4096, np.float32)
    _gen(case, "bias" + tag, 4096, np.float32)


def _cdesc(case, d, x, y, shape, k, tag="", stride=1, act=2, hint=0, cout=None):
    n, h, w, c = shape
    d.x, d.y = case.view(x, n, h, w, c, F16), case.view(y, n, h, w, cout or c, F16)
    d.w, d.scale, d.bias = case.addr("w" + tag), case.addr("scale" + tag), case.addr("bias" + tag)
    d.R = d.S = k
    d.stride, d.pad, d.act, d.tile_hint = stride, k // 2, act, hint
    return d


CSP_POINTERS = tuple(k + q for q in ("12", "m1", "m2", "3") for k in ("w", "scale", "bias"))      # by name, not by position


def _conv_cases():
    _lib, lib = _binding()
    out = []
    S = (2, 9, 11, 64)

    def conv2d(l, c, st):
        return l.glsdet_conv2d(C.byref(_cdesc(c, _lib.ConvDesc(), "x", "y", S, 3)), st)
    c = Case("conv2d", "glsdet_conv2d", conv2d)
    _conv_bufs(c, ["x", "y"]), _wsb(c, "")
    out.append(c)

    def multi(l, c, st):
        ds = (_lib.ConvDesc * 2)()
        _cdesc(c, ds[0], "x0", "y0", S, 3), _cdesc(c, ds[1], "x1", "y1", S, 3)
        return l.glsdet_conv2d_multi(ds, 2, st)
    c = Case("conv2d_multi", "glsdet_conv2d_multi", multi)
    _conv_bufs(c, ["x0", "x1", "y0", "y1"]), _wsb(c, "")
    out.append(c)

    def chain(l, c, st):
        ch = _lib.ConvChain()
        ch.y2 = c.view("y2", *S, F16)
        ch.w2, ch.scale2, ch.bias2 = c.addr("w2"), c.addr("scale2"), c.addr("bias2")
        ch.act2, ch.c0, ch.cin2, ch.flags = 2, 0, 64, 0
        return l.glsdet_conv2d_chain(C.byref(_cdesc(c, _lib.ConvDesc(), "x", "y", S, 3)), C.byref(ch), st)
    c = Case("conv2d_chain", "glsdet_conv2d_chain", chain)
    _conv_bufs(c, ["x", "y", "y2"]), _wsb(c, ""), _wsb(c, "2")
    out.append(c)

    def gnstats(l, c, st):
        return l.glsdet_conv2d_gnstats(C.byref(_cdesc(c, _lib.ConvDesc(), "x", "y", S, 3, act=0, hint=10)), 8, c.addr("stats"), st)
    c = Case("conv2d_gnstats", "glsdet_conv2d_gnstats", gnstats)
    _conv_bufs(c, ["x", "y"]), _wsb(c, "")
    c.buf("stats", lib.glsdet_conv2d_gnstats_bytes(2, 9, 11, 8), "out")
    out.append(c)

    for tag, shape in (("", S), ("@2x19x23", (2, 19, 23, 64))):        # dynamic LDS: two extents
        def bneck(l, c, st, shape=shape):
            d1 = _cdesc(c, _lib.ConvDesc(), "x", "hid", shape, 1, "1")
            d2 = _cdesc(c, _lib.ConvDesc(), "hid", "y", shape, 3, "2")
            return l.glsdet_bottleneck(C.byref(d1), C.byref(d2), 0, st)
        c = Case("bottleneck" + tag, "glsdet_bottleneck", bneck)
        _conv_bufs(c, ["x", "hid", "y"], shape), _wsb(c, "1"), _wsb(c, "2")
        out.append(c)

    for tag, shape in (("", (2, 9, 17, 64)), ("@2x19x23", (2, 19, 23, 64))):
        def csp(l, c, st, shape=shape):
            d = _lib.CspDesc()
            d.x, d.y, d.act, d.shortcut = c.view("x", *shape, F16), c.view("y", *shape, F16), 1, 1
            for k in CSP_POINTERS:
                setattr(d, k, c.addr(k))
            return l.glsdet_csp_fused(C.byref(d), 0, st)
        c = Case("csp_fused" + tag, "glsdet_csp_fused", csp)
        _conv_bufs(c, ["x", "y"], shape)
        assert {k for k, t in _lib.CspDesc._fields_ if t is C.c_void_p} == set(CSP_POINTERS)
        for k in CSP_POINTERS:
            _gen(c, k, RAW_BYTES if k.startswith("w") else 4096, np.float16 if k.startswith("w") else np.float32)
        out.append(c)

    G = (2, 6, 8, 64)

    def grouped(l, c, st):
        return l.glsdet_conv2d_grouped(C.byref(_cdesc(c, _lib.ConvDesc(), "x", "y", G, 3, act=1)), 8, st)
    c = Case("conv2d_grouped", "glsdet_conv2d_grouped", grouped)
    _conv_bufs(c, ["x", "y"], G), _wsb(c, "", max(RAW_BYTES, 2 * lib.glsdet_conv_grouped_weight_elems(8, 8)))
    out.append(c)

    D = (2, 9, 11, 16)

    def dw(l, c, st):
        return l.glsdet_dwconv2d(C.byref(_cdesc(c, _lib.ConvDesc(), "x", "y", D, 3, act=2)), st)
    c = Case("dwconv2d", "glsdet_dwconv2d", dw)
    _conv_bufs(c, ["x", "y"], D), _wsb(c, "")
    out.append(c)
    _exact_conv_data({q.key: q for q in out})
    return out


# ---- the exact regime of tests/conv_reference.py (ternary operands, scale 1 + j 2^-11, bias m 2^-11: every fp32 step exact, one
# rounding to fp16) on the geometry of the cases above, a seed per data set; weights packed on the host as
# glsdet_amd.torch_ops.pack_conv_weight packs them.  The reference's value replaces the generic data of the buffers named.
def _nhwc16(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).transpose(0, 2, 3, 1)).astype(np.float16)


def _packed(w, scale, bias, tag=""):
    import torch
    from glsdet_amd import torch_ops
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    flat, sc, bi = torch_ops.pack_conv_weight(t(w), t(scale), t(bias), w.shape[1], torch.float16, device="cpu")
    return {"w" + tag: flat.numpy(), "scale" + tag: sc.numpy(), "bias" + tag: bi.numpy()}


def _stage(key, shape, cout, ks, act, x=None, wkey=None):
    """one conv of the regime -> (x, w, scale, bias, float64 value before the rounding)"""
    from tests import conv_reference as R
    n, h, w, cin = shape
    wkey = key if wkey is None else wkey
    x = R.ternary((n, cin, h, w), 11, *key) if x is None else x
    wt = R.ternary((cout, cin, ks, ks), 12, *wkey)
    scale, bias = R.scale_bias(cout, *wkey)
    return x, wt, scale, bias, R.check_regime(R.conv(x, wt, 1, ks // 2), scale, bias, None, act)


def _second(key, stored, cout, ks, act):
    """a conv on stored values (tests/conv_reference.py check_second_regime) -> (w, scale, bias, value)"""
    from tests import conv_reference as R
    x2 = np.asarray(stored, np.float64)
    w2 = R.ternary((cout, x2.shape[1], ks, ks), 45, *key)
    s2, b2 = R.second_scale_bias(cout, 46, *key)
    return w2, s2, b2, R.check_second_regime(x2, w2, R.conv(x2, w2, 1, ks // 2), s2, b2, None, act, False, 1, ks // 2)


def _exact_conv_data(cases):
    from tests import conv_reference as R

    def wire(case, make, wants):
        data = lambda k: _once(("conv exact", case.key, k), lambda: make(k))
        for name, b in case.bufs.items():
            if b.role == "in":
                b.data = lambda k, name=name: data(k)[name]
        case._want = lambda k, outs: [m for name in wants for m in _cmp(name, outs[name], data(k)[name])]
        case.note = "" if set(wants) == {n for n, b in case.bufs.items() if b.role == "out"} else \
            "held to tests/conv_reference.py in %s; the other outputs to the immediate launch" % ", ".join(wants)

    S = (2, 9, 11, 64)

    def conv2d(k):
        x, w, sc, bi, v = _stage((k, 1), S, 64, 3, "relu")
        return dict(_packed(w, sc, bi), x=_nhwc16(x), y=_nhwc16(R.round_to(v, "f16")))
    wire(cases["conv2d"], conv2d, ["y"])

    def multi(k):
        d = {}
        for i in (0, 1):
            x, w, sc, bi, v = _stage((k, 2, i), S, 64, 3, "relu", wkey=(k, 2))
            d.update(_packed(w, sc, bi), **{"x%d" % i: _nhwc16(x), "y%d" % i: _nhwc16(R.round_to(v, "f16"))})
        return d
    wire(cases["conv2d_multi"], multi, ["y0", "y1"])

    def chain(k):
        x, w, sc, bi, v = _stage((k, 3), S, 64, 3, "relu")
        y = R.round_to(v, "f16")
        w2, s2, b2, v2 = _second((k, 3), y, 64, 1, "relu")
        return dict(_packed(w, sc, bi), **_packed(w2, s2, b2, "2"), x=_nhwc16(x), y=_nhwc16(y), y2=_nhwc16(R.round_to(v2, "f16")))
    wire(cases["conv2d_chain"], chain, ["y", "y2"])

    def gnstats(k):
        x, w, sc, bi, v = _stage((k, 4), S, 64, 3, "none")
        return dict(_packed(w, sc, bi), x=_nhwc16(x), y=_nhwc16(R.round_to(v, "f16")))
    wire(cases["conv2d_gnstats"], gnstats, ["y"])

    for key, shape in (("bottleneck", S), ("bottleneck@2x19x23", (2, 19, 23, 64))):
        def bneck(k, shape=shape):
            x, w1, s1, b1, v1 = _stage((k, 5) + shape, shape, 64, 1, "relu")
            hid = R.round_to(v1, "f16")
            w2, s2, b2, v2 = _second((k, 5) + shape, hid, 64, 3, "relu")
            return dict(_packed(w1, s1, b1, "1"), **_packed(w2, s2, b2, "2"), x=_nhwc16(x), y=_nhwc16(R.round_to(v2, "f16")))
        wire(cases[key], bneck, ["y"])

    D = (2, 9, 11, 16)

    def dw(k):
        x = R.ternary((2, 16, 9, 11), 21, k)
        w = R.ternary((16, 1, 3, 3), 22, k)
        sc, bi = R.scale_bias(16, 23, k)
        v = R.check_regime(R.conv(x, w, 1, 1, 1, depthwise=True), sc, bi, None, "relu")
        return {"w": np.ascontiguousarray(w.reshape(16, 9).T).astype(np.float16), "scale": sc.astype(np.float32), "bias": bi.astype(np.float32),
                "x": _nhwc16(x), "y": _nhwc16(R.round_to(v, "f16"))}
    wire(cases["dwconv2d"], dw, ["y"])


# ======================================================================================================== the non-local family
def _nonlocal_cases():
    """The exact regime of tests/nonlocal_reference.py (ternary theta / phi / g, Wout ternary * 2^-10, x and bias in eighths:
    every accumulation an exact integer number of steps), its expected() as the reference: one static window, the four
    quadrants of a map (scalar and matrix-core entry, the latter also on three windows of an 8 x 16 map), and the device-side split on the
    24 x 36 map with three different splits.  A data set is the same case under another name and seed."""
    from tests import nonlocal_reference as NR
    _lib, lib = _binding()
    out = []
    ci, cx, n = 64, 96, 2

    def make(key, entry, bases):
        """bases: the reference's Case per data set (one geometry)"""
        base = bases[0]
        split = base.kind == "split"
        FH, FW, tw = base.FH, base.FW, base.tw
        nsets = len(NR.windows(base))
        sets = [b._replace(name="replay-%s-set%d-%s" % (key, k, b.name), seed=b.seed + 17 * k) for k, b in enumerate(bases)]

        def data(k):
            def build():
                d = NR.case_data(sets[k])
                NR.check_regime(sets[k], d)
                return d
            return _once(("nonlocal", key, k), build)

        def win(c, name, ch, h0, h1, w0, w1):
            v = c.view(name, n, FH, FW, ch, F16)
            v.base += (h0 * FW + w0) * ch * 2
            v.h, v.w = h1 - h0, w1 - w0
            return v

        def call(l, c, st):
            wins = NR.windows(base) if not split else [(0, FH, 0, FW)]          # the split entry takes full maps
            arr = lambda name, ch, per_set=False: (_lib.View * len(wins if not split or not per_set else range(4)))(
                *[win(c, name + (str(q) if per_set else ""), ch, *wq) for q, wq in enumerate(wins if not split or not per_set else [wins[0]] * 4)])
            ptrs = lambda nm: (C.c_void_p * nsets)(*[c.addr("%s%d" % (nm, q)) for q in range(nsets)])
            if entry == "nonlocal":
                return l.glsdet_nonlocal(arr("x", cx), arr("t", tw), ci, c.addr("w0"), c.addr("b0"), c.addr("ws"), arr("o", cx), st)
            if entry == "nonlocal_multi":
                return l.glsdet_nonlocal_multi(arr("x", cx), arr("t", tw), nsets, ci, ptrs("w"), ptrs("b"), c.addr("ws"), arr("o", cx), st)
            if split:
                return l.glsdet_nonlocal_split(arr("x", cx), arr("t", tw, True), ci, ptrs("w"), ptrs("b"), c.addr("ws"), arr("o", cx),
                                               c.addr("split"), base.shift, st)
            return l.glsdet_nonlocal_mfma(arr("x", cx), arr("t", tw), nsets, ci, ptrs("w"), ptrs("b"), c.addr("ws"), c.nbytes("ws"),
                                          arr("o", cx), st)

        def want(k, outs):
            v = NR.expected(sets[k]).transpose(0, 2, 3, 1)                      # NaN where no set writes
            full = _ff(v.shape, np.float16)
            full[~np.isnan(v)] = v[~np.isnan(v)].astype(np.float16)
            return _cmp("o", outs["o"], full)
        c = Case(key, "glsdet_" + entry, call, n_sets=len(bases), want=want)
        c.buf("x", n * FH * FW * cx * 2, "in", lambda k: _nhwc16(data(k)["x"]))
        c.buf("o", n * FH * FW * cx * 2, "out")
        for q in range(4 if split else 1):
            c.buf("t%s" % (q if split else ""), n * FH * FW * tw * 2, "in", lambda k, q=q: _nhwc16(np.nan_to_num(data(k)["tpg"][q], nan=7.0)))
        for q in range(nsets):
            c.buf("w%d" % q, cx * ci * 4, "in", lambda k, q=q: np.asarray(data(k)["wout"][q], np.float32))
            c.buf("b%d" % q, cx * 4, "in", lambda k, q=q: np.asarray(data(k)["bout"][q], np.float32))
        if entry == "nonlocal_mfma":
            c.buf("ws", lib.glsdet_nonlocal_mfma_workspace_bytes(n, nsets, ci, cx), "ws")
        else:
            c.buf("ws", 4 * _lib.nonlocal_workspace_floats(nsets, n, ci, cx), "ws")
        if split:
            c.buf("split", 16, "in", lambda k: np.array(tuple(sets[k].split) + (0,), np.int32))
        out.append(c)

    two = lambda case: [case, case]
    make("nonlocal", "nonlocal", two(NR._static("static-4x4", ci, cx, 4, 4, n, "dense", "dense", "dense")))
    make("nonlocal_multi", "nonlocal_multi", two(NR._multi("quadrants-4x5", ci, cx, 4, 5, NR.quadrants(4, 5), n, "dense", "dense", "dense")))
    make("nonlocal_mfma", "nonlocal_mfma", two(NR._multi("quadrants-4x5", ci, cx, 4, 5, NR.quadrants(4, 5), n, "dense", "dense", "dense")))
    make("nonlocal_mfma@8x16", "nonlocal_mfma", two(NR._multi("three-8x16", ci, cx, 8, 16, [(0, 4, 0, 8), (4, 8, 0, 8), (0, 8, 8, 16)], n, "dense", "dense", "dense")))
    make("nonlocal_split", "nonlocal_split", [NR._split(ci, cx, n, sp, 0, "dense", "dense", "dense") for sp in ((12, 18, 22), (4, 5, 7), (20, 32, 5))])
    return out


# ========================================================================================================== post-processing
def _ff(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = 0xFF
    return a


def _as(b, dtype, shape):
    return b[: int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape)


def _cmp(name, got, want):
    g, w = np.ascontiguousarray(got).reshape(-1).view(np.uint8), np.ascontiguousarray(want).reshape(-1).view(np.uint8)
    return [] if np.array_equal(g, w) else ["%s differs from the reference in %d bytes" % (name, int((g != w).sum()))]


_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _nhwc32(x_nchw):
    """fp32 NCHW -> fp32 NHWC with the channels zero padded to a multiple of 8 (tests/test_resdet.py _fp32_view)"""
    x = np.asarray(x_nchw, np.float32)
    n, c, h, w = x.shape
    out = np.zeros((n, h, w, (c + 7) // 8 * 8), np.float32)
    out[..., :c] = x.transpose(0, 2, 3, 1)
    return out


def _decode_case(ex):
    _lib, lib = _binding()
    n, nc, sizes, strides = 2, 3, ((8, 11), (4, 5), (2, 3)), (8, 16, 32)
    A = sum(h * w for h, w in sizes)

    def call(l, c, st):
        arr = (_lib.View * 3)(*[c.view("l%d" % i, n, h, w, 8, F32) for i, (h, w) in enumerate(sizes)])
        sv = (C.c_int32 * 3)(*strides)
        if ex:
            return l.glsdet_yolox_decode_ex(arr, 3, nc, 64, 96, sv, 1, 2, c.addr("out"), n * A * 8, c.addr("sf"), st)
        return l.glsdet_yolox_decode(arr, 3, nc, 64, 96, sv, 1, c.addr("out"), n * A * 8, c.addr("sf"), st)

    def want(k, outs):
        """tests/decode_reference.py: the float64 formula within BOUND on |err| / (|x| + 1), the rule of tests/test_post_fuzz.py"""
        import torch
        from tests import decode_reference as D
        lv = [torch.from_numpy(c.host("l%d" % i, k).view(np.float32).reshape(n, h, w, 8).transpose(0, 3, 1, 2).copy()) for i, (h, w) in enumerate(sizes)]
        sf = torch.from_numpy(c.host("sf", k).view(np.float32).reshape(n, 4).copy())
        ref = D.decode_f64(lv, nc, 64, 96, list(strides), 1, sf, 2 if ex else 3)
        got = _as(outs["out"], np.float32, (n, A, 8))
        err = D.rel_err(got, ref) if np.isfinite(got).all() else float("inf")
        return [] if err <= D.BOUND else ["out: max |err| / (|x| + 1) = %.3e against the float64 formula, bound %.0e" % (err, D.BOUND)]
    c = Case("yolox_decode_ex" if ex else "yolox_decode", "glsdet_yolox_decode_ex" if ex else "glsdet_yolox_decode", call, want=want)
    for i, (h, w) in enumerate(sizes):
        _gen(c, "l%d" % i, n * h * w * 8 * 4, np.float32)
    c.buf("sf", n * 4 * 4, "in", lambda k: np.float32([[1.5, 1.25, 1.5, 1.25], [0.5, 0.5, 0.5, 0.5]]) * (k + 1))
    c.buf("out", n * A * 8 * 4, "out")
    return c


def _nms_case():
    from tests import post_reference as R
    _lib, lib = _binding()
    A, nc, cap, M = R.A_DEFAULT, 10, 8192, (5000, 70, 0)
    pred = lambda k: _once(("nms", k), lambda: R.to_pred([R.build_image(A, nc, M[k], scores="few", seed=80 + k)], nc, 1))

    def call(l, c, st):
        return l.glsdet_nms(c.addr("pred"), 1, A, nc, 1, R.CONF_THR, 0.5, cap, cap, c.addr("dets"), c.addr("count"), c.addr("status"),
                            c.addr("ws"), c.nbytes("ws"), st)

    def want(k, outs):
        ref = _once(("nms ref", k), lambda: R.reference_dets(pred(k)[0], nc, 1, 0.5))
        K = len(ref)
        return (_cmp("dets", _as(outs["dets"], np.float32, (cap, 7))[:K], np.asarray(ref, np.float32)) +
                _cmp("count", _as(outs["count"], np.int32, (2,)), np.int32([min(K, cap), K])) +
                _cmp("status", _as(outs["status"], np.int32, (1,)), np.int32([0])))
    c = Case("nms", "glsdet_nms", call, n_sets=3, want=want)
    c.buf("pred", A * (5 + nc) * 4, "in", pred)
    c.buf("dets", cap * 7 * 4, "out").buf("count", 8, "out").buf("status", 4, "out")
    c.buf("ws", lib.glsdet_nms_workspace_bytes(1, A, cap), "ws")
    return c


def _pack_detections_case():
    n, max_det, cap = 3, 12, 8
    kept, total = ([12, 9, 3], [2, 0, 1], [0, 0, 0]), ([40, 9, 3], [2, 0, 1], [0, 0, 0])
    dets = lambda k: np.random.default_rng(40 + k).uniform(-5, 700, (n, max_det, 7)).astype(np.float32)

    def call(l, c, st):
        return l.glsdet_pack_detections(c.addr("dets"), c.addr("count"), n, max_det, cap, c.addr("out"), st)

    def want(k, outs):
        w = np.zeros((n, cap + 1, 7), np.float32)
        for i in range(n):
            m = min(kept[k][i], max_det, cap)
            w[i, :m] = dets(k)[i, :m]
            w[i, cap, 0], w[i, cap, 1] = m, total[k][i]
        return _cmp("out", _as(outs["out"], np.float32, w.shape), w)
    c = Case("pack_detections", "glsdet_pack_detections", call, n_sets=3, want=want)
    c.buf("dets", n * max_det * 7 * 4, "in", dets)
    c.buf("count", 2 * n * 4, "in", lambda k: np.int32(kept[k] + total[k]))
    c.buf("out", n * (cap + 1) * 7 * 4, "out")
    return c


def _gfl_sets():
    """GFL_CASES[0] at bias -3 (many) and -8 (few), and a set with no score above the threshold"""
    import torch
    from tests import test_post_fuzz as PF

    def make(k):
        case = dict(PF.GFL_CASES[0], bias=(-3.0, -8.0, -3.0)[k], seed=PF.GFL_CASES[0]["seed"] + 10 * k)
        cls, reg = PF._gfl_inputs(case, 2)
        if k == 2:
            cls = [torch.full_like(t, -30.0) - torch.rand(t.shape, generator=torch.Generator().manual_seed(5)) for t in cls]
        return [_nhwc32(t.numpy()) for t in cls], [_nhwc32(t.numpy()) for t in reg]
    return lambda k: _once(("gfl", k), lambda: make(k))


GFL_HW = ([[290, 400], [296, 424]], [[280, 390], [296, 420]], [[296, 424], [250, 300]])


def _gfl_case(detect):
    from tests import test_post_fuzz as PF
    _lib, lib = _binding()
    case, n, L = PF.GFL_CASES[0], 2, 5
    nc, rm, max_cand, nms_pre, max_det = case["nc"], case["reg_max"], 2 * PF.MAX_CAND, case["nms_pre"], case["maxdet"]
    cap = sum(min(nms_pre, h * w * nc) for h, w in PF.GFL_SIZES)
    sets = _gfl_sets()
    cc, rc = (nc + 7) // 8 * 8, (4 * (rm + 1) + 7) // 8 * 8

    def call(l, c, st):
        ca = (_lib.View * L)(*[c.view("cls%d" % i, n, h, w, cc, F32) for i, (h, w) in enumerate(PF.GFL_SIZES)])
        ra = (_lib.View * L)(*[c.view("reg%d" % i, n, h, w, rc, F32) for i, (h, w) in enumerate(PF.GFL_SIZES)])
        sv = (C.c_int32 * L)(*PF.GFL_STRIDES)
        if detect:
            return l.glsdet_gfl_detect(ca, ra, L, sv, nc, rm, PF.GFL_IN[0], PF.GFL_IN[1], c.addr("hw"), c.addr("sf"), case["thr"], nms_pre,
                                       case["iou"], max_cand, max_det, c.addr("dets"), c.addr("count"), c.addr("status"), c.addr("ws"),
                                       c.nbytes("ws"), st)
        return l.glsdet_gfl_candidates(ca, ra, L, sv, nc, rm, PF.GFL_IN[0], PF.GFL_IN[1], c.addr("hw"), case["thr"], nms_pre, max_cand,
                                       c.addr("cand"), cap, c.addr("count"), c.addr("status"), c.addr("ws"), c.nbytes("ws"), st)

    def want(k, outs):
        """(no bit-exact reference of the rows: tests/test_post_fuzz.py bounds them) no level overflows max_cand -- the rows
        would then depend on the order of arrival -- and the counts are many, few and none"""
        cnt = _as(outs["count"], np.int32, (n,))
        ok = (cnt > 50).all() if k == 0 else (cnt == 0).all() if k == 2 else ((cnt > 0) & (cnt < 50)).all()
        return _cmp("status", _as(outs["status"], np.int32, (1,)), np.int32([0])) + ([] if ok else ["counts %s of set %d" % (cnt.tolist(), k)])
    c = Case("gfl_detect" if detect else "gfl_candidates", "glsdet_gfl_detect" if detect else "glsdet_gfl_candidates", call, n_sets=3, want=want)
    for i, (h, w) in enumerate(PF.GFL_SIZES):
        c.buf("cls%d" % i, n * h * w * cc * 4, "in", lambda k, i=i: sets(k)[0][i])
        c.buf("reg%d" % i, n * h * w * rc * 4, "in", lambda k, i=i: sets(k)[1][i])
    c.buf("hw", n * 2 * 4, "in", lambda k: np.float32(GFL_HW[k]))
    if detect:
        c.buf("sf", n * 4 * 4, "in", lambda k: np.float32(PF.GFL_SF) * (1 + k))
        c.buf("dets", n * max_det * 7 * 4, "out").buf("count", 2 * n * 4, "out").buf("status", 4, "out")
        c.buf("ws", lib.glsdet_gfl_workspace_bytes(n, L, max_cand, nms_pre), "ws")
    else:
        c.buf("cand", n * cap * 8 * 4, "out").buf("count", n * 4, "out").buf("status", 4, "out")
        c.buf("ws", lib.glsdet_gfl_candidates_workspace_bytes(n, L, max_cand), "ws")
    return c


def _cand_rows(seed, counts, cap, nc=3):
    """candidate rows [n][cap][8] of tests/softnms_cases.dyadic_rows, counts[b] valid rows per image; the rest is noise"""
    from tests.softnms_cases import dyadic_rows
    rows = [dyadic_rows(seed + b, m, nc) for b, m in enumerate(counts)]
    host = np.random.default_rng(seed).uniform(-50, 50, (len(counts), cap, 8)).astype(np.float32)
    for b, r in enumerate(rows):
        host[b, : len(r), :6] = r
    return host, rows


def _soft_nms_case(cap, counts, with_want):
    from tests import softnms_reference as S
    _lib, lib = _binding()
    n, nc = len(counts[0]), 3
    data = lambda k: _once(("softnms", cap, k), lambda: _cand_rows(100 * cap + 10 * k, counts[k], cap, nc))

    def call(l, c, st):
        return l.glsdet_soft_nms(c.addr("cand"), c.addr("cnt"), n, cap, nc, S.METHODS["hard"], 0.3, 0.5, 1e-4, 0, cap, c.addr("dets"),
                                 c.addr("count"), c.addr("status"), c.addr("ws"), c.nbytes("ws"), st)

    def want(k, outs):
        dets, count, bad = _as(outs["dets"], np.float32, (n, cap, 7)), np.zeros(2 * n, np.int32), []
        for b, r in enumerate(data(k)[1]):
            d, K, _ = S.detections(np.asarray(r, np.float32).reshape(-1, 6), S.METHODS["hard"], 0.3, 0.5, 1e-4, False, cap)
            count[b], count[n + b] = len(d), K
            bad += _cmp("dets of image %d" % b, dets[b, : len(d)], np.asarray(d, np.float32).reshape(-1, 7))
        return bad + _cmp("count", _as(outs["count"], np.int32, (2 * n,)), count) + _cmp("status", _as(outs["status"], np.int32, (1,)), np.int32([0]))
    c = Case("soft_nms@cap%d" % cap, "glsdet_soft_nms", call, n_sets=3, want=want if with_want else None)
    c.buf("cand", n * cap * 8 * 4, "in", lambda k: data(k)[0])
    c.buf("cnt", n * 4, "in", lambda k: np.int32(counts[k]))
    c.buf("dets", n * cap * 7 * 4, "out").buf("count", 2 * n * 4, "out").buf("status", 4, "out")
    c.buf("ws", lib.glsdet_soft_nms_workspace_bytes(n, cap), "ws")
    return c


def _aug_merge_case():
    from tests import tta_reference as T
    _lib, lib = _binding()
    n, K, caps, max_det, iou = 1, 2, (160, 96), 100, 0.5
    counts = ((150, 90), (5, 3), (0, 0))
    metas = lambda k: [(64.0 + 4 * k, 72.0 + 4 * k, [1.0, 1.0, 1.0, 1.0], 0), (64.0 + 4 * k, 72.0 + 4 * k, [2.0, 2.0, 2.0, 2.0], 1 + k)]
    scale = lambda k: np.float32([[0.5 * (k + 1)] * 4])
    data = lambda k, a: _once(("aug", k, a), lambda: _cand_rows(700 + 10 * k + a, [counts[k][a]], caps[a]))

    def call(l, c, st):
        pa = (C.c_void_p * K)(c.addr("cand0"), c.addr("cand1"))
        pc = (C.c_void_p * K)(c.addr("cnt0"), c.addr("cnt1"))
        cp = (C.c_int32 * K)(*caps)
        return l.glsdet_aug_merge_nms(pa, pc, cp, K, n, c.addr("meta"), iou, max_det,
                                      c.addr("scale"), c.addr("dets"), c.addr("count"), c.addr("status"), c.addr("ws"), c.nbytes("ws"), st)

    def want(k, outs):
        d, total, _ = T.merge([data(k, a)[1][0] for a in range(K)], metas(k), iou, max_det, scale(k)[0])
        return (_cmp("dets", _as(outs["dets"], np.float32, (max_det, 7))[: len(d)], d) +
                _cmp("count", _as(outs["count"], np.int32, (2,)), np.int32([len(d), total])) +
                _cmp("status", _as(outs["status"], np.int32, (1,)), np.int32([0])))

    def meta(k):
        return np.float32([[[h, w] + sf + [code, 0]] for h, w, sf, code in metas(k)])
    c = Case("aug_merge_nms", "glsdet_aug_merge_nms", call, n_sets=3, want=want)
    for a in range(K):
        c.buf("cand%d" % a, n * caps[a] * 8 * 4, "in", lambda k, a=a: data(k, a)[0])
        c.buf("cnt%d" % a, n * 4, "in", lambda k, a=a: np.int32([counts[k][a]]))
    c.buf("meta", K * n * 8 * 4, "in", meta).buf("scale", n * 4 * 4, "in", scale)
    c.buf("dets", n * max_det * 7 * 4, "out").buf("count", 2 * n * 4, "out").buf("status", 4, "out")
    c.buf("ws", lib.glsdet_aug_merge_workspace_bytes(n, (C.c_int32 * K)(*caps), K), "ws")
    return c


def _ufp_scene():
    from tests.test_ufp import _scene
    return _once("ufp scene", lambda: _scene(5))


def _ufp_chips(k):
    """the chips of tests/test_ufp.py's scene 5, floored; sets 1 and 2 move every source rectangle that has room by k pixels"""
    img, chips, cw, ch = _ufp_scene()
    c = np.floor(np.asarray(chips, np.float64)).astype(np.float32).reshape(-1, 7)
    H, W = img.shape[:2]
    room = (c[:, 0] + c[:, 2] + k < W - 1) & (c[:, 1] + c[:, 3] + k < H - 1)
    c[room, 0] += k
    c[room, 1] += k
    return c


def _ufp_merge_case():
    from tests import test_post_fuzz as PF
    _lib, lib = _binding()
    _, chips, cw, ch = _ufp_scene()
    rows = lambda k: _once(("ufp rows", k), lambda: PF._ufp_rows(_ufp_chips(k), cw, 5 + k))
    max_det, n_chips, max_cand = len(rows(0)) + 9, len(chips), 4096
    counts = (len(rows(0)), 6, 0)

    def dets(k):
        d = np.random.default_rng(k).uniform(0, 300, (max_det, 7)).astype(np.float32)
        d[: len(rows(k))] = rows(k)
        return d

    def call(l, c, st):
        return l.glsdet_ufp_backmap_merge(c.addr("dets"), c.addr("count"), max_det, c.addr("chips"), n_chips, 0.9, 0.6, max_cand, max_cand,
                                          c.addr("out"), c.addr("out_count"), c.addr("status"), c.addr("ws"), c.nbytes("ws"), st)

    def want(k, outs):
        """oracle.ufp_oracle.map_back_and_merge under the rule of tests/test_post_fuzz.py: per class the same number of rows,
        rtol 1e-5 / atol 1e-3 on the five columns; the status word 0"""
        from oracle import ufp_oracle as U
        used = np.asarray(rows(k)[: counts[k]], np.float32).reshape(-1, 7)
        ref = U.map_back_and_merge(PF._per_class(used, 3), [list(map(float, r)) for r in _ufp_chips(k)], num_classes=3)
        cnt = _as(outs["out_count"], np.int32, (2,))
        bad = _cmp("status", _as(outs["status"], np.int32, (1,)), np.int32([0]))
        if cnt[0] != sum(len(r) for r in ref) or cnt[1] != cnt[0]:
            return bad + ["out_count %s, the reference keeps %d" % (cnt.tolist(), sum(len(r) for r in ref))]
        got = _as(outs["out"], np.float32, (max_cand, 7))[: cnt[0]]
        for cls in range(3):
            g = got[got[:, 6] == cls][:, :5].astype(np.float64)
            if len(g) != len(ref[cls]) or (len(g) and not np.allclose(g, ref[cls], rtol=1e-5, atol=1e-3)):
                bad.append("class %d: %d rows against %d of the reference, or rows beyond the tolerance" % (cls, len(g), len(ref[cls])))
        return bad
    c = Case("ufp_backmap_merge", "glsdet_ufp_backmap_merge", call, n_sets=3, want=want)
    c.buf("dets", max_det * 7 * 4, "in", dets).buf("count", 8, "in", lambda k: np.int32([counts[k]] * 2))
    c.buf("chips", n_chips * 7 * 4, "in", _ufp_chips)
    c.buf("out", max_cand * 7 * 4, "out").buf("out_count", 8, "out").buf("status", 4, "out")
    c.buf("ws", lib.glsdet_ufp_merge_workspace_bytes(max_cand), "ws")
    return c


def _ufp_pack_case():
    from tests import test_ufp_pack_fuzz as UP
    n_img, max_det = 2, 75
    sizes = ((70, 23), (4, 1), (0, 0))
    scenes = lambda k: _once(("ufp pack", k), lambda: [UP.fixed_scene(10 * k + i + 1, m) for i, m in enumerate(sizes[k])])

    def call(l, c, st):
        return l.glsdet_ufp_pack(c.addr("dets"), c.addr("count"), n_img, max_det, 1.5, 1360, 765, c.addr("chips"), c.addr("floor"),
                                 c.addr("header"), c.addr("status"), st)

    def want(k, outs):
        wants = [(len(s[0]), UP.want_of(("replay", k, i), s)) for i, s in enumerate(scenes(k))]
        chips, floor = _ff((n_img, max_det, 7), np.float64), _ff((n_img, max_det, 7), np.float32)
        header, status = np.zeros((n_img, 4)), np.zeros(n_img, np.int32)
        for i, (n_boxes, (cc, cw, ch)) in enumerate(wants):
            cc = np.asarray(cc, np.float64).reshape(-1, 7)
            chips[i, : len(cc)], floor[i, : len(cc)], header[i] = cc, np.floor(cc).astype(np.float32), [n_boxes, len(cc), cw, ch]
        return (_cmp("chips", _as(outs["chips"], np.float64, chips.shape), chips) + _cmp("floor", _as(outs["floor"], np.float32, floor.shape), floor) +
                _cmp("header", _as(outs["header"], np.float64, header.shape), header) + _cmp("status", _as(outs["status"], np.int32, (n_img,)), status))
    c = Case("ufp_pack", "glsdet_ufp_pack", call, n_sets=3, want=want)
    c.buf("dets", n_img * max_det * 7 * 4, "in", lambda k: UP.dets_of(scenes(k), max_det, seed=k)[0])
    c.buf("count", n_img * 4, "in", lambda k: UP.dets_of(scenes(k), max_det, seed=k)[1])
    c.buf("chips", n_img * max_det * 7 * 8, "out").buf("floor", n_img * max_det * 7 * 4, "out")
    c.buf("header", n_img * 4 * 8, "out").buf("status", n_img * 4, "out")
    return c


def _voc_ap_case():
    """three row scenes of one geometry (the sizes are host arguments): 40 ground truths and 60, 60, 60 detections of other
    seeds; the thresholds differ"""
    from tests import test_vocap_fuzz as VF
    _lib, lib = _binding()
    THR = ([0.5, 0.75], [0.3, 0.5], [0.4, 0.6])
    scene = lambda k: _once(("voc", k), lambda: (lambda gt_dr: gt_dr + (VF.prepare(*gt_dr),))(VF.row_scene(40, 60, 900 + k)))
    h0 = scene(0)[2]
    T, ND, NC, NG, P = 2, h0["ND"], len(h0["classes"]), len(h0["gt_difficult"]), len(h0["pair_off"]) - 1
    ins = ("dt_box", "score", "cls_off", "pair_off", "pair_det", "gt_off", "gt_box", "gt_difficult", "n_gt", "n_img")
    outs_ = (("tp", np.int32, (T, ND)), ("fp", np.int32, (T, ND)), ("rec", np.float64, (T, ND)), ("prec", np.float64, (T, ND)),
             ("mpre", np.float64, (T, ND)), ("cls_out", np.float64, (T, NC, 16)))

    def call(l, c, st):
        a = c.addr
        return l.glsdet_voc_ap(a("dt_box"), a("score"), a("cls_off"), ND, NC, a("pair_off"), a("pair_det"), a("gt_off"), P, a("gt_box"),
                               a("gt_difficult"), NG, a("n_gt"), a("n_img"), a("thr"), T, a("fppi"), a("tp"), a("fp"), a("rec"), a("prec"),
                               a("mpre"), a("cls_out"), a("ws"), c.nbytes("ws"), st)

    def want(k, outs):
        gt, dr, h = scene(k)
        bad = []
        for (name, dt, shape), w in zip(outs_, VF.expected(gt, dr, THR[k], h)):
            bad += _cmp(name, _as(outs[name], dt, shape), np.asarray(w, dt))
        return bad
    c = Case("voc_ap", "glsdet_voc_ap", call, n_sets=3, want=want, note="one geometry in all three sets: every size is a host argument")
    for name in ins:
        a0 = np.ascontiguousarray(h0[name])
        c.buf(name, a0.nbytes, "in", lambda k, name=name, a0=a0: _same_size(scene(k)[2][name], a0))
    c.buf("thr", T * 8, "in", lambda k: np.float64(THR[k]))
    c.buf("fppi", 72, "in", lambda k: np.logspace(-2.0, 0.0, num=9))
    for name, dt, shape in outs_:
        c.buf(name, int(np.prod(shape)) * np.dtype(dt).itemsize, "out")
    c.buf("ws", max(int(lib.glsdet_voc_ap_workspace_bytes(NG, T)), 256), "ws")
    return c


def _same_size(a, a0):
    a = np.ascontiguousarray(a)
    assert a.nbytes == a0.nbytes and a.dtype == a0.dtype, "the sets of one case share their geometry"
    return a


def _coco_match_case():
    """three (image, category) pairs in buffers for 12 detections and 9 ground truths; the offsets, which live on the device,
    describe many, few and no boxes"""
    P, ND, NG, A, T = 3, 12, 9, 2, 2
    DT = ([0, 5, 9, 12], [0, 1, 1, 3], [0, 0, 0, 0])
    GT = ([0, 4, 6, 9], [0, 2, 2, 3], [0, 0, 0, 0])
    NI = 37

    def boxes(k, m, seed):
        r = np.random.default_rng([seed, k])
        b = np.concatenate([r.integers(0, 40, (m, 2)), r.integers(4, 30, (m, 2))], 1).astype(np.float64)
        return b, b[:, 2] * b[:, 3]

    def iou_off(k):
        d, g = np.diff(DT[k]), np.diff(GT[k])
        return np.concatenate([[0], np.cumsum(d * g)]).astype(np.int64)
    assert iou_off(0)[-1] == NI

    def call(l, c, st):
        a = c.addr
        return l.glsdet_coco_match(a("dt_box"), a("dt_area"), a("dt_off"), a("gt_box"), a("gt_area"), a("gt_flags"), a("gt_off"), a("iou_off"),
                                   P, ND, NG, a("area_rng"), A, a("iou_thr"), T, a("ious"), a("gt_order"), a("gt_ignore"), a("n_regular"),
                                   a("dt_match"), a("dt_ignore"), a("gt_match"), st)
    c = Case("coco_match", "glsdet_coco_match", call, n_sets=3)
    c.buf("dt_box", ND * 32, "in", lambda k: boxes(k, ND, 1)[0]).buf("dt_area", ND * 8, "in", lambda k: boxes(k, ND, 1)[1])
    c.buf("gt_box", NG * 32, "in", lambda k: boxes(k, NG, 2)[0]).buf("gt_area", NG * 8, "in", lambda k: boxes(k, NG, 2)[1])
    c.buf("gt_flags", NG, "in", lambda k: np.random.default_rng([3, k]).integers(0, 4, NG).astype(np.uint8))
    c.buf("dt_off", (P + 1) * 4, "in", lambda k: np.int32(DT[k])).buf("gt_off", (P + 1) * 4, "in", lambda k: np.int32(GT[k]))
    c.buf("iou_off", (P + 1) * 8, "in", iou_off)
    c.buf("area_rng", A * 16, "in", lambda k: np.float64([[0, 1e10], [0, 200.0 + 100 * k]]))
    c.buf("iou_thr", T * 8, "in", lambda k: np.float64([0.5, 0.75]) - 0.1 * k)
    c.buf("ious", NI * 8, "out").buf("gt_order", A * NG * 4, "out").buf("gt_ignore", A * NG, "out").buf("n_regular", A * P * 4, "out")
    c.buf("dt_match", A * T * ND * 4, "out").buf("dt_ignore", A * T * ND, "out").buf("gt_match", A * T * NG * 4, "out")
    return c


# ================================================================================================================= images
def _image_cases():
    from glsdet_amd import preprocess as PP
    from tests.test_preprocess import synth_image
    _lib, lib = _binding()
    out = []
    ih, iw, oh, ow, H, W, oy, ox = 37, 53, 45, 61, 64, 64, 3, 2
    xb, xk, xks = PP.pil_bicubic_tables(iw, ow)
    yb, yk, yks = PP.pil_bicubic_tables(ih, oh)

    def pil(l, c, st):
        a = c.addr
        return l.glsdet_pil_resize_normalize(a("src"), ih, iw, a("xb"), a("xk"), xks, ow, a("yb"), a("yk"), yks, oh, a("tmp"), a("dst"), H, W, oy, ox,
                                             (C.c_double * 3)(*PP.MEAN), (C.c_double * 3)(*PP.STD), st)

    def pil_want(k, outs):
        """tests/image_reference.py: Pillow's two passes and preprocess_input, pasted at (oy, ox); the rest of the canvas is the caller's"""
        from tests import image_reference as IR
        full = _ff((3, H, W), np.float32)
        full[:, oy: oy + oh, ox: ox + ow] = IR.normalize_drone(IR.two_pass(synth_image((ih, iw), 20 + k), (oh, ow)))
        return _cmp("dst", outs["dst"], full)
    c = Case("pil_resize_normalize", "glsdet_pil_resize_normalize", pil, want=pil_want, note="the coefficient tables follow from the sizes: the same in both sets")
    c.buf("src", ih * iw * 3, "in", lambda k: synth_image((ih, iw), 20 + k))
    for nm, t in (("xb", xb), ("xk", xk), ("yb", yb), ("yk", yk)):
        c.buf(nm, t.nbytes, "in", lambda k, t=t: t)
    c.buf("tmp", ih * ow * 3, "ws").buf("dst", 3 * H * W * 4, "out")
    out.append(c)

    img0, chips0, cw, ch = _ufp_scene()
    mh, mw = img0.shape[:2]
    cH, cW, nchips = max(1, int(np.ceil(ch))), max(1, int(np.ceil(cw))), len(chips0)

    def mosaic(l, c, st):
        return l.glsdet_ufp_mosaic(c.addr("img"), mh, mw, c.addr("chips"), nchips, c.addr("canvas"), cH, cW, st)

    def mosaic_want(k, outs):
        """oracle.ufp_oracle.display_merge_result, the rule of tests/test_image_fuzz.py: exact, zero outside the chips"""
        from oracle import ufp_oracle as U
        img = np.ascontiguousarray(synth_image((mh, mw), 5 + k)[:, :, ::-1])
        w = U.display_merge_result(img, [list(map(float, r)) for r in _ufp_chips(k)], cw, ch)
        assert w.shape == (cH, cW, 3)
        return _cmp("canvas", outs["canvas"], w.astype(np.float32))
    c = Case("ufp_mosaic", "glsdet_ufp_mosaic", mosaic, want=mosaic_want)
    c.buf("img", mh * mw * 3, "in", lambda k: np.ascontiguousarray(synth_image((mh, mw), 5 + k)[:, :, ::-1]))
    c.buf("chips", nchips * 7 * 4, "in", _ufp_chips).buf("canvas", cH * cW * 3 * 4, "out")
    out.append(c)

    h, w, nh, nw, ph, pw = 37, 53, 45, 61, 64, 64
    for name, u8, flip in (("resize_normalize_pad", False, None), ("resize_normalize_pad_u8", True, None),
                           ("resize_normalize_pad_ex", False, 3), ("resize_normalize_pad_u8_ex", True, 1)):
        def rnp(l, c, st, name=name, flip=flip):
            from tests import image_reference as IR
            m, s = (C.c_double * 3)(*IR.MEAN_RGB), (C.c_double * 3)(*IR.STD_RGB)
            args = (c.addr("src"), h, w, nh, nw, c.addr("dst"), ph, pw, m, s) + (() if flip is None else (flip,)) + (st,)
            return getattr(l, "glsdet_" + name)(*args)

        def rnp_want(k, outs, u8=u8, flip=flip):
            """oracle.ufp_oracle.resize_normalize, exactly (tests/test_image_fuzz.py); a flip mirrors the nh x nw window
            (tests/test_tta_fuzz.py); the padding is zero"""
            from oracle import ufp_oracle as U
            src = synth_image((h, w), 30 + k)
            src = src if u8 else src.astype(np.float32) + np.float32(0.25 * (k + 1))
            want = np.zeros((3, ph, pw), np.float32)
            win = U.resize_normalize(src, nw, nh)
            for axis, bit in ((2, 1), (1, 2)):
                if (flip or 0) & bit:
                    win = np.flip(win, axis)
            want[:, :nh, :nw] = win
            return _cmp("dst", outs["dst"], want)
        c = Case(name, "glsdet_" + name, rnp, want=rnp_want)
        if u8:
            c.buf("src", h * w * 3, "in", lambda k: synth_image((h, w), 30 + k))
        else:
            c.buf("src", h * w * 3 * 4, "in", lambda k: synth_image((h, w), 30 + k).astype(np.float32) + np.float32(0.25 * (k + 1)))
        c.buf("dst", 3 * ph * pw * 4, "out")
        out.append(c)

    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_sweep_420_rst.jpg"), "rb") as f:
        data = f.read()
    d0 = _lib.JpegDesc()
    src = (C.c_ubyte * len(data)).from_buffer_copy(data)
    assert lib.glsdet_jpeg_parse(C.cast(src, C.c_void_p), len(data), C.byref(d0)) == 0
    nb, row = int(d0.n_blocks), 3 * d0.width + 5

    def jpeg(l, c, st):
        d = _lib.JpegDesc.from_buffer_copy(d0)
        return l.glsdet_jpeg_reconstruct(C.byref(d), c.addr("coef"), c.addr("qtab"), c.addr("ws"), c.nbytes("ws"), c.addr("dst"), row, 0, st)

    def jpeg_want(k, outs):
        from tests import jpeg_reference as JR
        info = JR.parse(data)
        coef = c.host("coef", k).view(np.int16).reshape(nb, 64)
        rgb = JR.reconstruct(info, coef, c.host("qtab", k).view(np.uint16).reshape(3, 64), "rgb")
        full = np.full((d0.height, row), 0xFF, np.uint8)             # the bytes of a row past 3 * width are not written
        full[:, : 3 * d0.width] = rgb.reshape(d0.height, 3 * d0.width)
        return _cmp("dst", outs["dst"], full)
    c = Case("jpeg_reconstruct", "glsdet_jpeg_reconstruct", jpeg, want=jpeg_want, note="the descriptor of tests/golden/jpeg_sweep_420_rst.jpg; coefficients in [-64, 64]")
    c.buf("coef", nb * 64 * 2, "in", lambda k: np.random.default_rng([9, k]).integers(-64, 65, nb * 64).astype(np.int16))
    c.buf("qtab", 3 * 64 * 2, "in", lambda k: np.random.default_rng([10, k]).integers(1, 17, 192).astype(np.uint16))
    c.buf("ws", lib.glsdet_jpeg_workspace_bytes(C.byref(d0)), "ws").buf("dst", d0.height * row, "out")
    out.append(c)
    return out


def _second_extent_cases():
    """the dynamic-LDS helpers at another extent than the Entry table's: lvc_encode 2 x 9 x 15 x 96, window_attention
    2 x 15 x 13 with 3 heads, window 7, shift 3 (a padded map)"""
    _lib, lib = _binding()

    def lvc(l, c, st):
        return l.glsdet_lvc_encode(C.byref(c.view("x", 2, 9, 15, 96, F16)), c.addr("cw"), c.addr("scale"), c.addr("ws"), c.nbytes("ws"),
                                   c.addr("E"), st)
    a = Case("lvc_encode@9x15x96", "glsdet_lvc_encode", lvc)
    _gen(a, "x", 2 * 9 * 15 * 96 * 2), _gen(a, "cw", 64 * 96 * 4, np.float32), _gen(a, "scale", 64 * 4, np.float32)
    a.buf("ws", lib.glsdet_lvc_encode_workspace_bytes(2, 9, 15, 96), "ws").buf("E", 2 * 64 * 96 * 4, "out")

    def wattn(l, c, st):
        return l.glsdet_window_attention(C.byref(c.view("qkv", 2, 15, 13, 288, F16)), C.byref(c.view("y", 2, 15, 13, 96, F16)), c.addr("table"),
                                         c.addr("qb"), 3, 7, 3, 0.125, st)
    b = Case("window_attention@15x13", "glsdet_window_attention", wattn)
    _gen(b, "qkv", 2 * 15 * 13 * 288 * 2), _gen(b, "table", RAW_BYTES, np.float32), _gen(b, "qb", 288 * 4, np.float32)
    _gen(b, "y", 2 * 15 * 13 * 96 * 2, role="out")
    return [a, b]


# =============================================================================================================== the registry
SOFT_COUNTS_128 = ((120, 60, 97), (5, 0, 3), (0, 0, 0))
SOFT_COUNTS_3000 = ((1500, 700, 300), (40, 0, 7), (0, 0, 0))        # the restatement is quadratic: about 2 s for these
STATEFUL = ("nms", "gfl_detect", "gfl_candidates", "aug_merge_nms", "ufp_backmap_merge", "ufp_pack", "soft_nms", "pack_detections", "voc_ap",
            "coco_match")
_cases = []


def cases():
    """every case, built once; each is bound by its user (bind_fake / bind_device)"""
    if not _cases:
        cs = _helper_cases() + _conv_cases() + _nonlocal_cases()
        cs += [_decode_case(False), _decode_case(True), _nms_case(), _pack_detections_case(), _gfl_case(True), _gfl_case(False),
               _aug_merge_case(), _soft_nms_case(128, SOFT_COUNTS_128, True), _soft_nms_case(3000, SOFT_COUNTS_3000, True),
               _ufp_merge_case(), _ufp_pack_case(), _voc_ap_case(), _coco_match_case()]
        cs += _image_cases() + _second_extent_cases()
        for c in cs:
            if not c.has_want and not c.note:
                c.note = NO_REFERENCE[c.export]
        _cases.extend(cs)
    return _cases


# why a case outside the helper table has no reference of its own
NO_REFERENCE = {
    "glsdet_csp_fused": "generic data: the layer is pinned to the four launches it replaces (tests/test_csp_fused.py); not wired here",
    "glsdet_conv2d_grouped": "generic data: the exact regime of tests/resnext_reference.py is not wired here",
    "glsdet_coco_match": "no restatement under tests/: the oracle (oracle/cocoeval_oracle.py) works on annotation dicts, not on these arrays",
    "glsdet_lvc_encode": NO_WANT["lvc_encode"], "glsdet_window_attention": NO_WANT["window_attention"],
}


def registry():
    """export -> its cases"""
    out = collections.OrderedDict()
    for c in cases():
        out.setdefault(c.export, []).append(c)
    return out
