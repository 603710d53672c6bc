"""float64 restatement of the YOLOX decode with its two selectors (glsdet_yolox_decode_ex): box format and sigmoid mask.
TEST INFRASTRUCTURE ONLY, shared by tests/test_drone_harness_import.py (CPU: it reproduces the reference's recorded
outputs) and tests/test_decode_modes.py (GPU: the kernels reproduce it).

The formula (drone/models/core/utils_bbox.py:36-306; mmdet yolox_head.py:298-308 for format 1 with explicit strides):
    cx = (t0 + gx) * s    cy = (t1 + gy) * s    w = exp(t2) * s    h = exp(t3) * s        s = strides[l], else in_h / H_l
    format 0: cx / in_w, cy / in_h, w / in_w, h / in_h        format 1: cx - w/2, cy - h/2, cx + w/2, cy + h/2 (/ scale)
    channel 4 -> sigmoid if mask & 1, channels 5.. -> sigmoid if mask & 2, else the logit itself."""
import torch

# the reference's function names -> (box format, sigmoid mask)
VARIANTS = {
    "decode_outputs": (0, 3),
    "decode_outputs_cls_sigmoid": (0, 2),
    "decode_outputs_no_sigmoid": (0, 1),
    "decode_outputs_no_sigmoid_all": (0, 0),
    "decode_outputs_xyxy": (1, 0),
}
# `decode_mode` of the reference harness (yolo.py:75-82) -> the function it selects
HARNESS_MODES = {"default": "decode_outputs", "obj_sigmoid": "decode_outputs_no_sigmoid",
                 "no_sigmoid": "decode_outputs_no_sigmoid_all", "cls_sigmoid": "decode_outputs_cls_sigmoid"}
BOUND = 1e-5               # on |err| / (|x| + 1): the project's decode bound (tests/test_post_fuzz.py)


def decode_f64(levels, nc, in_h, in_w, strides=None, mode=0, sf=None, sigmoid=3):
    """levels: [n, >= 5 + nc, h, w] tensors -> float64 [n, A, 5 + nc]"""
    out = []
    for l, x in enumerate(levels):
        n, c, h, w = x.shape
        p = x.double().permute(0, 2, 3, 1).reshape(n, h * w, c)[..., : 5 + nc].clone()
        s = float(strides[l]) if strides is not None else in_h / h
        gy, gx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        cx, cy = (p[..., 0] + gx.flatten()) * s, (p[..., 1] + gy.flatten()) * s
        bw, bh = torch.exp(p[..., 2]) * s, torch.exp(p[..., 3]) * s
        if mode == 0:
            p[..., 0], p[..., 1], p[..., 2], p[..., 3] = cx / in_w, cy / in_h, bw / in_w, bh / in_h
        else:
            box = torch.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], -1)
            p[..., :4] = box / sf.double()[:, None, :] if sf is not None else box
        if sigmoid & 1:
            p[..., 4] = torch.sigmoid(p[..., 4])
        if sigmoid & 2:
            p[..., 5:] = torch.sigmoid(p[..., 5:])
        out.append(p)
    return torch.cat(out, 1)


def rel_err(got, want):
    """max |got - want| / (|want| + 1) in float64"""
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    return float(((got - want).abs() / (want.abs() + 1.0)).max())
