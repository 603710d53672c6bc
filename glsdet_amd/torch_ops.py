"""torch custom ops over the C ABI: `torch.ops.glsdet.*` (north_star: "the hot path ... exposed through torch
custom ops"; SURVEY section 8b, C-ABI / custom-op layer).

Each op is one C-ABI call of libglsdet_hip.so on the CURRENT HIP stream of the input's device: inputs are borrowed
(they must be contiguous in the declared layout, else RuntimeError -- the reference's assertion style), outputs are
allocated by the op on the input's device, nothing synchronises.  There is no CPU implementation: a CPU tensor raises.

    glsdet::conv_bn_act(x, w, scale, bias, cout, R, S, stride, pad, act, res=None, out_fp32=False) -> y
        x NHWC [N,H,W,C] (C % 8 == 0) fp16 or fp32; w = pack_conv_weight(...) ; scale / bias fp32 [cout_pad];
        y NHWC [N,Ho,Wo,ceil8(cout)];  act: 0 none 1 silu 2 relu 3 lrelu 4 gelu 5 sigmoid (| 0x100 residual first)
        reference: BaseConv drone/models/base/baseConv.py:6-19 (+ Bottleneck add, darknet.py:61-62)
        limit: the conv reads x through 32-bit descriptor offsets counted from the start of x's STORAGE, so an x whose
        storage is 2 GiB or more (2^31 - 1 bytes) is refused ("exceeds the 2 GiB descriptor range") even when x itself is
        a small slice of it, e.g. one image of a large batch tensor: clone() the slice first
    glsdet::conv2d_grouped(x, w, scale, bias, groups, stride, act) -> y
        grouped 3x3 conv, pad 1, stride 1 / 2, C = groups * Cg with Cg in 4 / 8 / 16 / 32; w, scale, bias =
        pack_conv_grouped_weight(...); y NHWC [N,Ho,Wo,C] in x's dtype
        reference: conv2 of the ResNeXt Bottleneck, ufp/mmdet/models/backbones/resnext.py:55-64
    glsdet::nonlocal_dot(x, tpg, ci, wout, bout) -> y
    glsdet::nonlocal_dot_mfma(x, tpg, ci, wout, bout) -> y     (the same on the matrix cores: ci, C multiples of 32)
        Non_local_Block without its three projections: drone/models/block/non_local/Identity_Conv.py:157-173
    glsdet::lvc_encode(x, codewords, scale) -> E fp32 [N, 64, C]
        the codebook Encoding layer, drone/models/cfp/Functions.py:25-84: x NHWC (C a multiple of 32, at most 640),
        codewords fp32 [64, C], scale fp32 [64]
    glsdet::lvc_gate(E, a, b, fc_w, fc_b) -> gam fp32 [N, C]
        BatchNorm1d per code (folded: a, b fp32 [64]) + ReLU + mean over the codes + fc + sigmoid, cfp/evc_blocks.py:223-238
    glsdet::channel_fuse(a, t, v, mode) -> y
        mode 0: relu(a + a * v[n, c]) (evc_blocks.py:239; t = None); mode 1: a + v[c] * t (evc_blocks.py:272)
    glsdet::yolox_decode(levels, num_classes, in_h, in_w, mode=0, sigmoid=3) -> pred [N, A, 5+nc]
        decode_outputs, drone/models/core/utils_bbox.py:254-306 (mode 1: mmdet YOLOXHead._bbox_decode); sigmoid: bit 0
        objectness, bit 1 classes, channels outside the mask stay raw logits (the variants of utils_bbox.py:36-253)
    glsdet::nms(pred, num_classes, box_mode, conf_thres, nms_thres, max_det) -> (dets [N,max_det,7], count [2N], status [1])
        class max + threshold + per-class NMS of non_max_suppression, utils_bbox.py:375-419
    glsdet::soft_nms(cand, counts, num_classes, method, iou_thr, sigma, min_score, rescore, max_det)
            -> (dets [N,max_det,7], count [2N], status [1])
        py_cpu_softnms / batched_soft_nms, drone/merge_results.py:41-130; cand fp32 [N, cap, 8] rows x1,y1,x2,y2,score,label,
        counts int32 [N]; method 1 linear, 2 gaussian, 3 hard; dets rows x1,y1,x2,y2, original score, decayed score, label
    glsdet::ufp_pack(dets, counts, expand, img_w, img_h) -> (chips f64 [N,max_det,7], chips_floor f32 [N,max_det,7],
            header f64 [N,4], status int32 [N])
        UnifiedForegroundPacking, ufp/UFPMP-Det-Tools/ufp/unified_foreground_packing.py:6-197 + spp.py:77-168, on the coarse
        detector's rows: dets fp32 [N, max_det, 7] x1,y1,x2,y2,score,score,label, counts int32 [N] (or the detector's [2N]);
        chip rows src_x,src_y,w,h,canvas_x,canvas_y,magnification; header n_boxes,n_chips,canvas_w,canvas_h
    glsdet::voc_ap(dt_box, score, cls_off, pair_off, pair_det, gt_off, gt_box, gt_difficult, n_gt, n_img, min_overlap,
            fppi_ref, validate=False) -> (tp i32 [T,ND], fp i32 [T,ND], rec f64 [T,ND], prec f64 [T,ND], mpre f64 [T,ND],
            cls_out f64 [T,C,16])
        VOC-style mAP, get_map of drone/models/core/utils_map.py:294-813 (matching :474-512, curves :570-617, voc_ap
        :99-140, the nine picked miss rates of :26-62); the arrays of glsdet_voc_ap in include/glsdet_hip.h, built by
        glsdet_amd/eval/voc.py.  validate=True reads the offsets back (one synchronisation) and refuses non-monotone
        offsets or a pair_det that is no permutation; the kernels clamp either way.
    glsdet::jpeg_reconstruct(coef, qtab, geometry, order) -> rgb uint8 [H, W, 3]
        the device half of the baseline JPEG decoder (glsdet_jpeg_reconstruct: dequantise, libjpeg's ISLOW inverse DCT,
        fancy upsampling, YCbCr -> RGB; what Image.open(path).convert("RGB") gives): coef int16 [n_blocks, 64] and qtab
        uint16 (or int16 bits) [3, 64] as glsdet_jpeg_entropy_decode leaves them, geometry = width, height, ncomp, hs[3],
        vs[3] (glsdet_amd.jpeg.geometry), order 0 RGB / 1 BGR
    glsdet::batched_nms(boxes, scores, idxs, iou_threshold) -> keep int64 [K]
        torchvision.ops.boxes.batched_nms's signature (utils_bbox.py:414-419), one image

Importing this module registers the ops (idempotent).  `pack_conv_weight` / `fold_bn` are host-side helpers.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import F16, F32, ConvDesc, View, check, nonlocal_workspace_floats

_DT = {torch.float16: F16, torch.float32: F32}


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _need_cuda(*ts):
    for t in ts:
        if t is not None and t.device.type != "cuda":
            raise RuntimeError("glsdet ops run on an MI355X only (got a %s tensor): there is no CPU fallback" % t.device.type)


def _nhwc_view(t: torch.Tensor, what: str) -> View:
    if t.dim() != 4 or not t.is_contiguous() or t.dtype not in _DT:
        raise RuntimeError("%s must be a contiguous NHWC [N,H,W,C] fp16 / fp32 tensor" % what)
    n, h, w, c = t.shape
    if c % 8:
        raise RuntimeError("%s: channels must be a multiple of 8 (got %d)" % (what, c))
    st = t.untyped_storage()
    return View(t.data_ptr(), h * w * c, w * c, c, n, h, w, c, _DT[t.dtype], 0, st.data_ptr(), st.data_ptr() + st.nbytes())


def ceil_to(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def pack_conv_weight(w: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, cin_pad: int, dtype: torch.dtype,
                     device="cuda") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """OIHW weights + per-channel scale / bias -> (packed [cout_pad, kpad] in `dtype`, scale fp32 [cout_pad], bias fp32
    [cout_pad]) as glsdet_conv2d wants them: k = (r*S + s)*cin_pad + ci, rows / K zero padded."""
    lib = _lib.load()
    cout, cin, R, S = w.shape
    assert cin <= cin_pad and cin_pad % 8 == 0
    kpad = lib.glsdet_conv_kpad(R, S, cin_pad, _DT[dtype])
    cpad = lib.glsdet_conv_cout_pad(ceil_to(cout, 8))
    wp = torch.zeros(cpad, R, S, cin_pad, dtype=torch.float32)
    wp[:cout, :, :, :cin] = w.detach().float().cpu().permute(0, 2, 3, 1)
    flat = torch.zeros(cpad, kpad, dtype=torch.float32)
    flat[:, : R * S * cin_pad] = wp.reshape(cpad, -1)
    sc, bi = torch.ones(cpad), torch.zeros(cpad)
    sc[:cout], bi[:cout] = scale.detach().float().cpu(), bias.detach().float().cpu()
    return flat.to(dtype).to(device), sc.to(device), bi.to(device)


def grouped_weight_blocks(w: torch.Tensor) -> torch.Tensor:
    """Grouped 3x3 weights [C, Cg, 3, 3] (C = groups * Cg, Cg in 4 / 8 / 16 / 32) -> the fp32 host image of
    glsdet_conv2d_grouped's operand: [ceil(C / 32), 9, 32, 32] = [block][tap r*3+s][co_l][ci_l], zero outside the diagonal
    Cg x Cg blocks and past C (include/glsdet_hip.h)."""
    C_, cg, R, S = w.shape
    if (R, S) != (3, 3) or cg not in (4, 8, 16, 32) or C_ % cg:
        raise ValueError("grouped_weight_blocks: [groups * Cg, Cg, 3, 3] with Cg in 4 / 8 / 16 / 32, got %s" % (tuple(w.shape),))
    nblk = (C_ + 31) // 32
    out = torch.zeros(nblk * 32, 9, 32, dtype=torch.float32)          # [co][tap][ci_l]
    wt = w.detach().float().cpu().permute(0, 2, 3, 1).reshape(C_, 9, cg)
    co = torch.arange(C_)
    ci_l = ((co // cg) * cg) % 32                                      # first column of co's group inside its block
    for j in range(cg):
        out[co, :, ci_l + j] = wt[:, :, j]
    return out.reshape(nblk, 32, 9, 32).permute(0, 2, 1, 3).contiguous()


def pack_conv_grouped_weight(w: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, dtype: torch.dtype,
                             device="cuda") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (grouped_weight_blocks(w) in `dtype`, scale fp32 [ceil32(C)], bias fp32 [ceil32(C)]) on `device`"""
    blocks = grouped_weight_blocks(w)
    cpad = blocks.shape[0] * 32
    sc, bi = torch.ones(cpad), torch.zeros(cpad)
    sc[:w.shape[0]], bi[:w.shape[0]] = scale.detach().float().cpu(), bias.detach().float().cpu()
    return blocks.to(dtype).to(device), sc.to(device), bi.to(device)


_REGISTERED = False


def register():
    global _REGISTERED
    if _REGISTERED:
        return
    _REGISTERED = True
    lib_def = torch.library.Library("glsdet", "DEF")
    lib_def.define("conv_bn_act(Tensor x, Tensor w, Tensor scale, Tensor bias, int cout, int R, int S, int stride, int pad, "
                   "int act, Tensor? res=None, bool out_fp32=False) -> Tensor")
    lib_def.define("conv2d_grouped(Tensor x, Tensor w, Tensor scale, Tensor bias, int groups, int stride, int act) -> Tensor")
    lib_def.define("nonlocal_dot(Tensor x, Tensor tpg, int ci, Tensor wout, Tensor bout) -> Tensor")
    lib_def.define("nonlocal_dot_mfma(Tensor x, Tensor tpg, int ci, Tensor wout, Tensor bout) -> Tensor")
    lib_def.define("lvc_encode(Tensor x, Tensor codewords, Tensor scale) -> Tensor")
    lib_def.define("lvc_gate(Tensor E, Tensor a, Tensor b, Tensor fc_w, Tensor fc_b) -> Tensor")
    lib_def.define("channel_fuse(Tensor a, Tensor? t, Tensor v, int mode) -> Tensor")
    lib_def.define("yolox_decode(Tensor[] levels, int num_classes, int in_h, int in_w, int mode=0, int sigmoid=3) -> Tensor")
    lib_def.define("nms(Tensor pred, int num_classes, int box_mode, float conf_thres, float nms_thres, int max_det) -> "
                   "(Tensor, Tensor, Tensor)")
    lib_def.define("soft_nms(Tensor cand, Tensor counts, int num_classes, int method, float iou_thr, float sigma, "
                   "float min_score, bool rescore, int max_det) -> (Tensor, Tensor, Tensor)")
    lib_def.define("ufp_pack(Tensor dets, Tensor counts, float expand, int img_w, int img_h) -> (Tensor, Tensor, Tensor, Tensor)")
    lib_def.define("voc_ap(Tensor dt_box, Tensor score, Tensor cls_off, Tensor pair_off, Tensor pair_det, Tensor gt_off, "
                   "Tensor gt_box, Tensor gt_difficult, Tensor n_gt, Tensor n_img, Tensor min_overlap, Tensor fppi_ref, "
                   "bool validate=False) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
    lib_def.define("jpeg_reconstruct(Tensor coef, Tensor qtab, int[] geometry, int order) -> Tensor")
    lib_def.define("batched_nms(Tensor boxes, Tensor scores, Tensor idxs, float iou_threshold) -> Tensor")
    impl = torch.library.Library("glsdet", "IMPL", "CUDA")
    cpu = torch.library.Library("glsdet", "IMPL", "CPU")
    meta = torch.library.Library("glsdet", "IMPL", "Meta")

    def no_cpu(*a, **k):
        raise RuntimeError("glsdet ops run on an MI355X only: there is no CPU fallback")

    # ------------------------------------------------------------------ conv_bn_act
    def conv_bn_act(x, w, scale, bias, cout, R, S, stride, pad, act, res=None, out_fp32=False):
        lib = _lib.load()
        _need_cuda(x, w, scale, bias, res)
        n, h, wd, c = x.shape
        ho, wo = (h + 2 * pad - R) // stride + 1, (wd + 2 * pad - S) // stride + 1
        ydt = torch.float32 if (out_fp32 or x.dtype == torch.float32) else x.dtype
        y = torch.empty(n, ho, wo, ceil_to(cout, 8), dtype=ydt, device=x.device)
        if w.dtype != x.dtype or not w.is_contiguous() or w.dim() != 2 or \
                w.shape[0] != lib.glsdet_conv_cout_pad(y.shape[3]) or w.shape[1] != lib.glsdet_conv_kpad(R, S, c, _DT[x.dtype]):
            raise RuntimeError("conv_bn_act: w must be pack_conv_weight(...)'s [cout_pad, kpad] matrix in x's dtype")
        if scale.dtype != torch.float32 or bias.dtype != torch.float32 or scale.numel() < w.shape[0] or bias.numel() < w.shape[0]:
            raise RuntimeError("conv_bn_act: scale / bias must be fp32 [cout_pad]")
        d = ConvDesc()
        d.x, d.y = _nhwc_view(x, "conv_bn_act.x"), _nhwc_view(y, "conv_bn_act.y")
        d.res = _nhwc_view(res, "conv_bn_act.res") if res is not None else View()
        d.w, d.scale, d.bias = w.data_ptr(), scale.data_ptr(), bias.data_ptr()
        d.R, d.S, d.stride, d.pad, d.act, d.tile_hint = R, S, stride, pad, act, 0
        check(lib.glsdet_conv2d(C.byref(d), _stream(x)), "conv_bn_act")
        return y

    def conv_bn_act_meta(x, w, scale, bias, cout, R, S, stride, pad, act, res=None, out_fp32=False):
        n, h, wd, c = x.shape
        ho, wo = (h + 2 * pad - R) // stride + 1, (wd + 2 * pad - S) // stride + 1
        return x.new_empty((n, ho, wo, ceil_to(cout, 8)), dtype=torch.float32 if out_fp32 else x.dtype)

    # ------------------------------------------------------------------ conv2d_grouped
    def conv2d_grouped(x, w, scale, bias, groups, stride, act):
        lib = _lib.load()
        _need_cuda(x, w, scale, bias)
        n, h, wd, c = x.shape
        y = torch.empty(n, (h - 1) // stride + 1, (wd - 1) // stride + 1, c, dtype=x.dtype, device=x.device)
        elems = lib.glsdet_conv_grouped_weight_elems(groups, c // groups if groups > 0 and c % groups == 0 else 0)
        if elems == 0 or w.dtype != x.dtype or not w.is_contiguous() or w.numel() != elems:
            raise RuntimeError("conv2d_grouped: w must be pack_conv_grouped_weight(...)'s [ceil(C/32), 9, 32, 32] blocks in x's "
                               "dtype, C = groups * Cg with Cg in 4 / 8 / 16 / 32")
        cpad = ceil_to(c, 32)
        if scale.dtype != torch.float32 or bias.dtype != torch.float32 or scale.numel() < cpad or bias.numel() < cpad:
            raise RuntimeError("conv2d_grouped: scale / bias must be fp32 [ceil32(C)]")
        d = ConvDesc()
        d.x, d.y, d.res = _nhwc_view(x, "conv2d_grouped.x"), _nhwc_view(y, "conv2d_grouped.y"), View()
        d.w, d.scale, d.bias = w.data_ptr(), scale.data_ptr(), bias.data_ptr()
        d.R, d.S, d.stride, d.pad, d.act, d.tile_hint = 3, 3, stride, 1, act, 0
        check(lib.glsdet_conv2d_grouped(C.byref(d), groups, _stream(x)), "conv2d_grouped")
        return y

    def conv2d_grouped_meta(x, w, scale, bias, groups, stride, act):
        n, h, wd, c = x.shape
        return x.new_empty((n, (h - 1) // stride + 1, (wd - 1) // stride + 1, c))

    # ------------------------------------------------------------------ nonlocal_dot
    def nonlocal_dot(x, tpg, ci, wout, bout):
        lib = _lib.load()
        _need_cuda(x, tpg, wout, bout)
        if wout.dtype != torch.float32 or bout.dtype != torch.float32 or not wout.is_contiguous() or \
                tuple(wout.shape) != (x.shape[3], ci) or bout.numel() != x.shape[3] or tpg.shape[3] < 3 * ci:
            raise RuntimeError("nonlocal_dot: wout fp32 [C, ci], bout fp32 [C], tpg NHWC with >= 3*ci channels")
        y = torch.empty_like(x)
        ws = torch.empty(nonlocal_workspace_floats(1, x.shape[0], ci, x.shape[3]), dtype=torch.float32, device=x.device)
        check(lib.glsdet_nonlocal(C.byref(_nhwc_view(x, "nonlocal_dot.x")), C.byref(_nhwc_view(tpg, "nonlocal_dot.tpg")), ci,
                                  wout.data_ptr(), bout.data_ptr(), ws.data_ptr(), C.byref(_nhwc_view(y, "nonlocal_dot.y")),
                                  _stream(x)), "nonlocal_dot")
        return y

    def nonlocal_dot_mfma(x, tpg, ci, wout, bout):
        """nonlocal_dot on the matrix-core kernels (glsdet_nonlocal_mfma: ci and C multiples of 32, at most 1280); a shape
        they do not take is an error here, not a switch to the other kernels"""
        lib = _lib.load()
        _need_cuda(x, tpg, wout, bout)
        if wout.dtype != torch.float32 or bout.dtype != torch.float32 or not wout.is_contiguous() or \
                tuple(wout.shape) != (x.shape[3], ci) or bout.numel() != x.shape[3] or tpg.shape[3] < 3 * ci:
            raise RuntimeError("nonlocal_dot_mfma: wout fp32 [C, ci], bout fp32 [C], tpg NHWC with >= 3*ci channels")
        y = torch.empty_like(x)
        nbytes = lib.glsdet_nonlocal_mfma_workspace_bytes(x.shape[0], 1, ci, x.shape[3])
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=x.device)
        xa, ta, ya = (View * 1)(_nhwc_view(x, "nonlocal_dot_mfma.x")), (View * 1)(_nhwc_view(tpg, "nonlocal_dot_mfma.tpg")), \
            (View * 1)(_nhwc_view(y, "nonlocal_dot_mfma.y"))
        wa, ba = (C.c_void_p * 1)(wout.data_ptr()), (C.c_void_p * 1)(bout.data_ptr())
        check(lib.glsdet_nonlocal_mfma(xa, ta, 1, ci, wa, ba, ws.data_ptr(), nbytes, ya, _stream(x)), "nonlocal_dot_mfma")
        return y

    # ------------------------------------------------------------------ EVC block (csrc/evc.hip)
    def _f32c(what, t, shape):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
            raise RuntimeError("%s must be a contiguous fp32 %s tensor, got %s %s" % (what, list(shape), t.dtype, tuple(t.shape)))

    def lvc_encode(x, codewords, scale):
        lib = _lib.load()
        _need_cuda(x, codewords, scale)
        xv = _nhwc_view(x, "lvc_encode.x")
        n, h, w, c = x.shape
        _f32c("lvc_encode: codewords", codewords, (64, c))
        _f32c("lvc_encode: scale", scale, (64,))
        nbytes = lib.glsdet_lvc_encode_workspace_bytes(n, h, w, c)
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=x.device)
        E = torch.empty(n, 64, c, dtype=torch.float32, device=x.device)
        check(lib.glsdet_lvc_encode(C.byref(xv), codewords.data_ptr(), scale.data_ptr(), ws.data_ptr(), nbytes, E.data_ptr(),
                                    _stream(x)), "lvc_encode")
        return E

    def lvc_gate(E, a, b, fc_w, fc_b):
        lib = _lib.load()
        _need_cuda(E, a, b, fc_w, fc_b)
        if E.dim() != 3 or E.shape[1] != 64:
            raise RuntimeError("lvc_gate: E must be fp32 [N, 64, C]")
        n, _, c = E.shape
        for what, t, shape in (("E", E, (n, 64, c)), ("a", a, (64,)), ("b", b, (64,)), ("fc_w", fc_w, (c, c)), ("fc_b", fc_b, (c,))):
            _f32c("lvc_gate: " + what, t, shape)
        gam = torch.empty(n, c, dtype=torch.float32, device=E.device)
        check(lib.glsdet_lvc_gate(E.data_ptr(), n, c, a.data_ptr(), b.data_ptr(), fc_w.data_ptr(), fc_b.data_ptr(), gam.data_ptr(),
                                  _stream(E)), "lvc_gate")
        return gam

    def channel_fuse(a, t, v, mode):
        lib = _lib.load()
        _need_cuda(a, t, v)
        n, _, _, c = a.shape
        _f32c("channel_fuse: v", v, (n, c) if mode == 0 else (c,))
        y = torch.empty_like(a)
        av, yv = _nhwc_view(a, "channel_fuse.a"), _nhwc_view(y, "channel_fuse.y")
        tv = C.byref(_nhwc_view(t, "channel_fuse.t")) if t is not None else None
        check(lib.glsdet_channel_fuse(C.byref(av), tv, C.byref(yv), v.data_ptr(), mode, _stream(a)), "channel_fuse")
        return y

    # ------------------------------------------------------------------ yolox_decode
    def yolox_decode(levels, num_classes, in_h, in_w, mode=0, sigmoid=3):
        lib = _lib.load()
        _need_cuda(*levels)
        if any(l.dtype != torch.float32 for l in levels):
            raise RuntimeError("yolox_decode: the head logits are fp32 NHWC levels")
        n = levels[0].shape[0]
        A = sum(l.shape[1] * l.shape[2] for l in levels)
        out = torch.empty(n, A, 5 + num_classes, dtype=torch.float32, device=levels[0].device)
        arr = (View * len(levels))(*[_nhwc_view(l, "yolox_decode.level") for l in levels])
        strides = (C.c_int32 * len(levels))(*[in_h // l.shape[1] for l in levels]) if mode == 1 else None
        check(lib.glsdet_yolox_decode_ex(arr, len(levels), num_classes, in_h, in_w, strides, mode, sigmoid, out.data_ptr(),
                                         out.numel(), None, _stream(out)), "yolox_decode")
        return out

    def yolox_decode_meta(levels, num_classes, in_h, in_w, mode=0, sigmoid=3):
        return levels[0].new_empty((levels[0].shape[0], sum(l.shape[1] * l.shape[2] for l in levels), 5 + num_classes))

    # ------------------------------------------------------------------ nms
    def nms(pred, num_classes, box_mode, conf_thres, nms_thres, max_det):
        lib = _lib.load()
        _need_cuda(pred)
        if pred.dtype != torch.float32 or not pred.is_contiguous() or pred.dim() != 3 or pred.shape[2] != 5 + num_classes:
            raise RuntimeError("nms: pred must be a contiguous fp32 [N, A, 5 + num_classes] tensor")
        n, A = pred.shape[0], pred.shape[1]
        ws = torch.empty(int(lib.glsdet_nms_workspace_bytes(n, A, A)), dtype=torch.uint8, device=pred.device)
        dets = torch.zeros(n, max_det, 7, dtype=torch.float32, device=pred.device)
        count = torch.zeros(2 * n, dtype=torch.int32, device=pred.device)
        status = torch.zeros(1, dtype=torch.int32, device=pred.device)
        check(lib.glsdet_nms(pred.data_ptr(), n, A, num_classes, box_mode, conf_thres, nms_thres, A, max_det, dets.data_ptr(),
                             count.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _stream(pred)), "nms")
        return dets, count, status

    def nms_meta(pred, num_classes, box_mode, conf_thres, nms_thres, max_det):
        n = pred.shape[0]
        return (pred.new_empty((n, max_det, 7)), pred.new_empty((2 * n,), dtype=torch.int32),
                pred.new_empty((1,), dtype=torch.int32))

    # ------------------------------------------------------------------ soft_nms
    def soft_nms(cand, counts, num_classes, method, iou_thr, sigma, min_score, rescore, max_det):
        lib = _lib.load()
        _need_cuda(cand, counts)
        if cand.dtype != torch.float32 or not cand.is_contiguous() or cand.dim() != 3 or cand.shape[2] != 8:
            raise RuntimeError("soft_nms: cand must be a contiguous fp32 [N, cap, 8] tensor")
        n, cap = cand.shape[0], cand.shape[1]
        if counts.dtype != torch.int32 or not counts.is_contiguous() or counts.numel() != n:
            raise RuntimeError("soft_nms: counts must be a contiguous int32 [N] tensor")
        ws = torch.empty(max(int(lib.glsdet_soft_nms_workspace_bytes(n, cap)), 256), dtype=torch.uint8, device=cand.device)
        dets = torch.zeros(n, max_det, 7, dtype=torch.float32, device=cand.device)
        count = torch.zeros(2 * n, dtype=torch.int32, device=cand.device)
        status = torch.zeros(1, dtype=torch.int32, device=cand.device)
        check(lib.glsdet_soft_nms(cand.data_ptr(), counts.data_ptr(), n, cap, num_classes, method, iou_thr, sigma, min_score,
                                  int(rescore), max_det, dets.data_ptr(), count.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                  ws.numel(), _stream(cand)), "soft_nms")
        return dets, count, status

    def soft_nms_meta(cand, counts, num_classes, method, iou_thr, sigma, min_score, rescore, max_det):
        n = cand.shape[0]
        return (cand.new_empty((n, max_det, 7)), cand.new_empty((2 * n,), dtype=torch.int32),
                cand.new_empty((1,), dtype=torch.int32))

    # ------------------------------------------------------------------ ufp_pack
    def ufp_pack(dets, counts, expand, img_w, img_h):
        lib = _lib.load()
        _need_cuda(dets, counts)
        if dets.dtype != torch.float32 or not dets.is_contiguous() or dets.dim() != 3 or dets.shape[2] != 7:
            raise RuntimeError("ufp_pack: dets must be a contiguous fp32 [N, max_det, 7] tensor")
        n, max_det = dets.shape[0], dets.shape[1]
        if counts.dtype != torch.int32 or not counts.is_contiguous() or counts.numel() not in (n, 2 * n):
            raise RuntimeError("ufp_pack: counts must be a contiguous int32 [N] (or the detector's [2N]) tensor")
        chips = torch.zeros(n, max_det, 7, dtype=torch.float64, device=dets.device)
        chips_floor = torch.zeros(n, max_det, 7, dtype=torch.float32, device=dets.device)
        header = torch.zeros(n, 4, dtype=torch.float64, device=dets.device)
        status = torch.zeros(n, dtype=torch.int32, device=dets.device)
        check(lib.glsdet_ufp_pack(dets.data_ptr(), counts.data_ptr(), n, max_det, expand, img_w, img_h, chips.data_ptr(),
                                  chips_floor.data_ptr(), header.data_ptr(), status.data_ptr(), _stream(dets)), "ufp_pack")
        return chips, chips_floor, header, status

    def ufp_pack_meta(dets, counts, expand, img_w, img_h):
        n, max_det = dets.shape[0], dets.shape[1]
        return (dets.new_empty((n, max_det, 7), dtype=torch.float64), dets.new_empty((n, max_det, 7)),
                dets.new_empty((n, 4), dtype=torch.float64), dets.new_empty((n,), dtype=torch.int32))

    # ------------------------------------------------------------------ voc_ap
    def _voc_shapes(dt_box, score, cls_off, pair_off, pair_det, gt_off, gt_box, gt_difficult, n_gt, n_img, min_overlap, fppi_ref):
        nd, ng, C_, P, T = score.numel(), gt_difficult.numel(), cls_off.numel() - 1, pair_off.numel() - 1, min_overlap.numel()
        for t, dt, shape, what in ((dt_box, torch.float64, (nd, 4), "dt_box fp64 [ND, 4]"), (score, torch.float64, (nd,), "score fp64 [ND]"),
                                   (cls_off, torch.int32, (C_ + 1,), "cls_off int32 [C+1]"), (pair_off, torch.int32, (P + 1,), "pair_off int32 [P+1]"),
                                   (pair_det, torch.int32, (nd,), "pair_det int32 [ND]"), (gt_off, torch.int32, (P + 1,), "gt_off int32 [P+1]"),
                                   (gt_box, torch.float64, (ng, 4), "gt_box fp64 [NG, 4]"),
                                   (gt_difficult, torch.uint8, (ng,), "gt_difficult uint8 [NG]"), (n_gt, torch.int32, (C_,), "n_gt int32 [C]"),
                                   (n_img, torch.int32, (C_,), "n_img int32 [C]"), (min_overlap, torch.float64, (T,), "min_overlap fp64 [T]"),
                                   (fppi_ref, torch.float64, (9,), "fppi_ref fp64 [9]")):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                raise RuntimeError("voc_ap: %s expected, got %s %s" % (what, t.dtype, tuple(t.shape)))
        if C_ < 0 or P < 0 or T < 1:
            raise RuntimeError("voc_ap: offsets need at least one entry and min_overlap at least one threshold")
        return nd, ng, C_, P, T

    def voc_ap(dt_box, score, cls_off, pair_off, pair_det, gt_off, gt_box, gt_difficult, n_gt, n_img, min_overlap, fppi_ref,
               validate=False):
        lib = _lib.load()
        args = (dt_box, score, cls_off, pair_off, pair_det, gt_off, gt_box, gt_difficult, n_gt, n_img, min_overlap, fppi_ref)
        _need_cuda(*args)
        nd, ng, C_, P, T = _voc_shapes(*args)
        if validate:
            for t, top, what in ((cls_off, nd, "cls_off"), (pair_off, nd, "pair_off"), (gt_off, ng, "gt_off")):
                h = t.cpu()
                if int(h[0]) != 0 or int(h[-1]) != top or bool((h[1:] < h[:-1]).any()):
                    raise RuntimeError("voc_ap: %s must rise from 0 to %d without a step down" % (what, top))
            if nd and not torch.equal(torch.sort(pair_det.cpu().long()).values, torch.arange(nd)):
                raise RuntimeError("voc_ap: pair_det must hold every detection index exactly once")
        dev = score.device
        ws = torch.empty(int(lib.glsdet_voc_ap_workspace_bytes(ng, T)), dtype=torch.uint8, device=dev)
        tp, fp = (torch.zeros(T, nd, dtype=torch.int32, device=dev) for _ in range(2))
        rec, prec, mpre = (torch.zeros(T, nd, dtype=torch.float64, device=dev) for _ in range(3))
        cls_out = torch.zeros(T, C_, 16, dtype=torch.float64, device=dev)
        ptr = lambda t: t.data_ptr() if t.numel() else None
        if C_ > 0:
            check(lib.glsdet_voc_ap(ptr(dt_box), ptr(score), cls_off.data_ptr(), nd, C_, pair_off.data_ptr(), ptr(pair_det),
                                    gt_off.data_ptr(), P, ptr(gt_box), ptr(gt_difficult), ng, n_gt.data_ptr(), n_img.data_ptr(),
                                    min_overlap.data_ptr(), T, fppi_ref.data_ptr(), ptr(tp), ptr(fp), ptr(rec), ptr(prec), ptr(mpre),
                                    cls_out.data_ptr(), ws.data_ptr(), ws.numel(), _stream(score)), "voc_ap")
        return tp, fp, rec, prec, mpre, cls_out

    def voc_ap_meta(dt_box, score, cls_off, pair_off, pair_det, gt_off, gt_box, gt_difficult, n_gt, n_img, min_overlap, fppi_ref,
                    validate=False):
        nd, C_, T = score.numel(), cls_off.numel() - 1, min_overlap.numel()
        i32, f64 = (lambda *s: score.new_empty(s, dtype=torch.int32)), (lambda *s: score.new_empty(s, dtype=torch.float64))
        return i32(T, nd), i32(T, nd), f64(T, nd), f64(T, nd), f64(T, nd), f64(T, C_, 16)

    # ------------------------------------------------------------------ jpeg_reconstruct (csrc/jpeg.hip)
    def jpeg_reconstruct(coef, qtab, geometry, order):
        from .jpeg import desc_from_geometry
        lib = _lib.load()
        _need_cuda(coef, qtab)
        d = desc_from_geometry(geometry)
        if coef.dtype != torch.int16 or not coef.is_contiguous() or coef.numel() != d.n_blocks * 64 or d.n_blocks < 1:
            raise RuntimeError("jpeg_reconstruct: coef must be a contiguous int16 [n_blocks, 64] tensor of the geometry's %d blocks"
                               % d.n_blocks)
        if qtab.dtype not in (torch.uint16, torch.int16) or not qtab.is_contiguous() or qtab.numel() != 192:
            raise RuntimeError("jpeg_reconstruct: qtab must be a contiguous uint16 [3, 64] tensor")
        out = torch.empty(d.height, d.width, 3, dtype=torch.uint8, device=coef.device)
        nws = lib.glsdet_jpeg_workspace_bytes(C.byref(d))
        ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=coef.device)
        check(lib.glsdet_jpeg_reconstruct(C.byref(d), coef.data_ptr(), qtab.data_ptr(), ws.data_ptr(), nws, out.data_ptr(),
                                          3 * d.width, order, _stream(coef)), "jpeg_reconstruct")
        return out

    # ------------------------------------------------------------------ batched_nms (torchvision's signature)
    def batched_nms(boxes, scores, idxs, iou_threshold):
        _need_cuda(boxes, scores, idxs)
        m = boxes.shape[0]
        if m == 0:
            return torch.zeros(0, dtype=torch.int64, device=boxes.device)
        if (scores < 0).any():
            raise RuntimeError("batched_nms: scores must be >= 0")
        lab = idxs.to(torch.int64)
        nc = int(lab.max().item()) + 1
        pred = torch.full((1, m, 5 + nc), -1.0, dtype=torch.float32, device=boxes.device)
        pred[0, :, :4] = boxes.float()
        pred[0, :, 4] = 1.0
        pred[0, torch.arange(m, device=boxes.device), 5 + lab] = scores.float()
        dets, count, _ = nms(pred, nc, 1, -0.5, float(iou_threshold), m)
        k = int(count[0].item())
        kept = dets[0, :k]
        rows = torch.cat([boxes.float(), scores.float()[:, None], lab.float()[:, None]], 1)            # [m, 6]
        got = torch.cat([kept[:, :4], (kept[:, 4] * kept[:, 5])[:, None], kept[:, 6:7]], 1)             # [k, 6]
        same = (got[:, None, :] == rows[None, :, :]).all(-1)                                            # [k, m]
        return torch.argmax(same.to(torch.int8), dim=1)          # first (lowest) index of the identical row

    for name, fn, fm in (("conv_bn_act", conv_bn_act, conv_bn_act_meta), ("conv2d_grouped", conv2d_grouped, conv2d_grouped_meta), ("nonlocal_dot", nonlocal_dot, lambda x, *a: torch.empty_like(x)),
                         ("nonlocal_dot_mfma", nonlocal_dot_mfma, lambda x, *a: torch.empty_like(x)),
                         ("lvc_encode", lvc_encode, lambda x, c, s: x.new_empty((x.shape[0], 64, x.shape[3]), dtype=torch.float32)),
                         ("lvc_gate", lvc_gate, lambda E, *a: E.new_empty((E.shape[0], E.shape[2]))),
                         ("channel_fuse", channel_fuse, lambda a, *r: torch.empty_like(a)),
                         ("yolox_decode", yolox_decode, yolox_decode_meta), ("nms", nms, nms_meta),
                         ("soft_nms", soft_nms, soft_nms_meta), ("ufp_pack", ufp_pack, ufp_pack_meta), ("voc_ap", voc_ap, voc_ap_meta),
                         ("jpeg_reconstruct", jpeg_reconstruct,
                          lambda coef, qtab, geometry, order: coef.new_empty((geometry[1], geometry[0], 3), dtype=torch.uint8)),
                         ("batched_nms", batched_nms, lambda b, s, i, t: b.new_empty((0,), dtype=torch.int64))):
        impl.impl(name, fn)
        cpu.impl(name, no_cpu)
        meta.impl(name, fm)
    register._libs = (lib_def, impl, cpu, meta)          # keep the registrations alive


register()
