"""CPU restatement of the reference's models/cfp/yolox_cfp.py forward (kind `cfp`), written from the formulas of the EVC block
and composed with functions of oracle.glsdet_oracle (imported only) for everything the plain YOLOX shares; the fixture it is
held against (tests/golden/cfp_golden.npz, tools/make_cfp_golden.py: the reference's own modules behind a stand-in for the
`timm` imports); the exact-regime builders and the a-priori bound of tests/test_lvc_exact.py.

    csp_darknet (BN eps 1e-3) -> lateral_conv0 -> up2 -> EVCBlock -> cat with dark4 -> the PAFPN lines of oracle.pafpn
    -> yolox_head, every BatchNorm of neck and head at eps 1e-5, the four of ConvBlock at 1e-6

Any dtype: pass a float64 state dict and input for the float64 evaluation.  Under oracle.fp16_storage() the tensors the HIP
path stores in fp16 are rounded where it stores them (the encoding, the gate vector and every per-channel vector stay fp32).

`mistakes`: a set of names from MISTAKES; each plants one wrong reading of the reference, for the tests that show that the
committed data would see it."""
import contextlib
import os

import numpy as np
import torch
import torch.nn.functional as F

from glsdet_amd.synth import synth_input, synth_state_dict
from oracle import glsdet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cfp_golden.npz")
SEED = 5
NUM_CLASSES = 10
NUM_CODES = 64
CASES = [("tiny", (2, 3, 128, 160)), ("tiny", (1, 3, 160, 224)), ("nano", (1, 3, 96, 160)), ("s", (1, 3, 64, 96))]
TABLE_PHIS = ("tiny", "nano", "s", "m")
F32_BAR = 1e-4                       # the floor of the GPU tests' f32 bar (tests/test_cross10.py)
SENSITIVITY = 1e-2                   # tools/make_cross10_golden.py: 100 x that bar
# erf and tanh GELU differ by 5e-4 at most: 1e-3 of the activations that any output is made of.  No linear gain changes that
# ratio, and a net chaotic enough to amplify it (gammas x 1.6 in the neck did, to 4e-2) sits 2e-4 from its own float64
# evaluation.  That one mistake is held at 10 x F32_BAR on the LightMLPBlock record instead.
MISTAKE_BAR = {"tanh_gelu": 1e-3}
# gains of the weight recipe, raised until every planted mistake moves its record by SENSITIVITY (tools/make_cfp_golden.py)
# while the reference's fp32 evaluation stays within 1e-6 of its float64 one
NECK_GAIN, EVC_GAIN, PRED_GAIN, FC1_GAIN, FC2_GAIN = 1.0, 3.0, 2.0, 2.0, 4.0
# block records: (name, C, h, w, batch)
ENCODING_RECORDS = [("enc_c32_n35", 32, 5, 7, 2), ("enc_c32_n130", 32, 10, 13, 2), ("enc_c96_n64", 96, 8, 8, 1)]
BLOCK_RECORDS = [("c32_6x10", 32, 6, 10, 2), ("c64_5x7", 64, 5, 7, 2)]
BLOCK_KINDS = ("lvc", "l_MLP", "evc")
# planted mistakes -> the record that must see each (a whole-model case index, or a block record)
MISTAKES = {"eps_neck_head_1e-3": ("case", 0), "eps_convblock_1e-5": ("block", "evc", 0), "softmax_over_pixels": ("encoding", 1),
            "drop_sum_term": ("encoding", 0), "scale_after_softmax": ("encoding", 2), "bn1d_per_channel": ("block", "evc", 1),
            "mean_over_channels": ("block", "evc", 1), "tanh_gelu": ("block", "l_MLP", 1), "drop_layer_scale": ("case", 0),
            "gate_without_x": ("case", 0), "no_maxpool": ("case", 0), "concat_swapped": ("case", 0),
            "evc_before_upsample": ("case", 0)}


def case_name(phi, shape):
    return "%s_%s" % (phi, "x".join(str(v) for v in shape))


_G = {}


def golden():
    if "g" not in _G:
        _G["g"] = np.load(GOLDEN)
    return _G["g"]


def table(phi):
    """the recorded {key: shape} of the reference module, in its order"""
    g = golden()
    names, shapes = g["table/%s/names" % phi], g["table/%s/shapes" % phi]
    return {str(k): tuple(int(v) for v in s if v >= 0) for k, s in zip(names, shapes)}


# ------------------------------------------------------------------------------------------------------------ weights
def recipe(sd):
    """The fixture's weight recipe on a synthesized state dict (in place; tools/make_cfp_golden.py explains why):
    the CSPDarknet's gammas x 0.5, those of neck and head x NECK_GAIN (what a SiLU takes away), evcblock.cnv1 x EVC_GAIN,
    the predictors' weights x PRED_GAIN, mlp.fc1 / fc2 weights x FC1_GAIN / FC2_GAIN; outside the CSPDarknet every BatchNorm2d's running_var is spread log-uniformly over
    [1e-3, 1] ([1e-5, 1e-2] in ConvBlock) with gamma scaled by sqrt(var) so that the layer's gain stays what it was -- a
    wrong eps then changes a channel's gain by up to 30 %; Encoding.scale in (-1, 0); BatchNorm1d's running_var at the
    scale of the encodings."""
    for k in list(sd):
        if k.endswith("bn.weight"):
            if k.startswith("backbone.backbone."):
                sd[k] = sd[k] * 0.5
            elif "evcblock." not in k and not k.startswith("blk."):
                sd[k] = sd[k] * NECK_GAIN
        if k.endswith("evcblock.cnv1.weight") or k.endswith("evcblock.cnv1.bias"):
            sd[k] = sd[k] * EVC_GAIN
        if "_preds." in k and k.endswith(".weight"):
            sd[k] = sd[k] * PRED_GAIN
        if k.endswith("mlp.fc1.weight"):
            sd[k] = sd[k] * FC1_GAIN
        if k.endswith("mlp.fc2.weight"):
            sd[k] = sd[k] * FC2_GAIN
    for k in list(sd):
        if not k.endswith("running_var") or k.startswith("backbone.backbone."):
            continue
        bn = k[: -len(".running_var")]
        if bn.endswith("LVC.4"):
            sd[k] = sd[k] * 4.0
            continue
        lo, hi = (-5.0, -2.0) if ".conv_1." in k else (-3.0, 0.0)
        var = 10.0 ** (lo + (hi - lo) * (sd[k] - 0.5))                 # synth: uniform(0.5, 1.5)
        sd[bn + ".weight"] = sd[bn + ".weight"] * var.sqrt()
        sd[bn + ".running_mean"] = sd[bn + ".running_mean"] * var.sqrt()
        sd[k] = var
    for k in list(sd):
        if k.endswith("LVC.3.scale"):
            sd[k] = -(sd[k] - 0.65) / 0.7                               # synth: uniform(0.7, 1.3) -> (-0.93, -0.07)
    return sd


def weights(phi):
    return recipe(synth_state_dict(table(phi), SEED))


def block_table(C):
    from glsdet_amd.arch import _Table, evc_table
    t = _Table()
    evc_table(t, "blk", C)
    return t


def block_weights(C):
    return recipe(synth_state_dict(block_table(C), SEED + C))


def case_input(phi, shape):
    return synth_input(shape, int(golden()["case/%s/seed" % case_name(phi, shape)]))


def recorded(phi, shape, which="out32"):
    g = golden()
    return [torch.from_numpy(g["case/%s/%s/%d" % (case_name(phi, shape), which, k)]) for k in range(3)]


def block_input(C, h, w, n, key=0):
    """non-negative, as the block sees it behind a ReLU / max pool only in the whole model; signed here"""
    return synth_input((n, C, h, w), 700 + C + key)


def block_recorded(kind, name, which="out32"):
    return torch.from_numpy(golden()["block/%s/%s/%s" % (kind, name, which)])


def to64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def rel(a, b):
    """max over the levels of |a - b| / max(1, |b|)"""
    if torch.is_tensor(a):
        a, b = [a], [b]
    return max(float(((u.double() - v.double()).abs() / v.double().abs().clamp(min=1)).max()) for u, v in zip(a, b))


# -------------------------------------------------------------------------------------------------------- restatement
@contextlib.contextmanager
def bn_eps(eps):
    """oracle.base_conv folds with the module constant BN_EPS: the neck and head of this kind run it at 1e-5"""
    old, O.BN_EPS = O.BN_EPS, eps
    try:
        yield
    finally:
        O.BN_EPS = old


def _bn(sd, p, x, eps):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, eps)


def _conv_bn(sd, conv, bn, x, pad, eps, act=True, res=None):
    """Conv2d(bias=False) + BatchNorm2d (+ res) + ReLU: one store of the HIP path"""
    y = _bn(sd, bn, F.conv2d(x, O._qw(sd[conv + ".weight"], conv), None, 1, pad), eps)
    if res is not None:
        y = y + res
    return O._q(torch.relu(y) if act else y, conv)


def encoding(x, codewords, scale, mistakes=()):
    """Encoding.forward by its definition: x [B, C, H, W] -> E [B, 64, C]
    A = softmax_k(s_k |x_n - c_k|^2),  E[b, k] = sum_n A[b, n, k] (x[b, n] - c[k])"""
    B, C = x.shape[:2]
    X = x.reshape(B, C, -1).transpose(1, 2)                             # [B, N, C]
    diff = X[:, :, None, :] - codewords[None, None]                     # [B, N, 64, C]
    d2 = diff.pow(2).sum(3)
    if "scale_after_softmax" in mistakes:
        A = torch.softmax(d2, 2) * scale
    else:
        A = torch.softmax(scale * d2, 1 if "softmax_over_pixels" in mistakes else 2)
    if "drop_sum_term" in mistakes:
        return (A[..., None] * X[:, :, None, :]).sum(1)
    return (A[..., None] * diff).sum(1)


def encoding_expanded(x, codewords, scale):
    """the same in the form the kernel evaluates: D = s (|x|^2 - 2 x.c + |c|^2), E = A^T X - (sum_n A) c"""
    B, C = x.shape[:2]
    X = x.reshape(B, C, -1).transpose(1, 2)
    D = scale * ((X.pow(2).sum(2, keepdim=True) - 2.0 * X @ codewords.t()) + codewords.pow(2).sum(1))
    A = torch.softmax(D, 2)
    return A.transpose(1, 2) @ X - A.sum(1)[:, :, None] * codewords


def lvc_block(sd, p, x, mistakes=()):
    """LVCBlock.forward: ConvBlock, the encoding branch down to the gate vector, relu(x + x * gam)"""
    q = p + ".conv_1"
    eps = 1e-5 if "eps_convblock_1e-5" in mistakes else 1e-6
    r = _conv_bn(sd, q + ".residual_conv", q + ".residual_bn", x, 0, eps, act=False)
    t = _conv_bn(sd, q + ".conv1", q + ".bn1", x, 0, eps)
    t = _conv_bn(sd, q + ".conv2", q + ".bn2", t, 1, eps)
    t = _conv_bn(sd, q + ".conv3", q + ".bn3", t, 0, eps, res=r)
    z = _conv_bn(sd, p + ".LVC.0", p + ".LVC.1", t, 0, 1e-5)
    E = encoding(z, sd[p + ".LVC.3.codewords"], sd[p + ".LVC.3.scale"], mistakes)          # [B, 64, C]
    bn = p + ".LVC.4"
    a = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + 1e-5)
    b = sd[bn + ".bias"] - sd[bn + ".running_mean"] * a
    if "bn1d_per_channel" in mistakes:                                  # (needs C == 64)
        en = torch.relu(E * a[None, None, :] + b[None, None, :])
    else:
        en = torch.relu(E * a[None, :, None] + b[None, :, None])
    en = en.mean(2) if "mean_over_channels" in mistakes else en.mean(1)
    gam = torch.sigmoid(F.linear(en, sd[p + ".fc.0.weight"], sd[p + ".fc.0.bias"]))[:, :, None, None]
    return O._q(torch.relu(t * gam if "gate_without_x" in mistakes else t + t * gam), p)


def light_mlp(sd, p, x, mistakes=()):
    """LightMLPBlock.forward; GroupNorm(1, C); dw = DWConv(ksize=1); exact-erf GELU; l_MLP.linear unused"""
    C = x.shape[1]
    ls = lambda i: sd["%s.layer_scale_%d" % (p, i)].reshape(1, C, 1, 1)
    g1 = O._q(F.group_norm(x, 1, sd[p + ".norm1.weight"], sd[p + ".norm1.bias"], 1e-5), p + ".norm1")
    y1 = O._q(x + ls(1) * O.dw_conv(sd, p + ".dw", g1), p + ".y1")
    if "drop_layer_scale" in mistakes:
        y1 = x + O.dw_conv(sd, p + ".dw", g1)
    g2 = O._q(F.group_norm(y1, 1, sd[p + ".norm2.weight"], sd[p + ".norm2.bias"], 1e-5), p + ".norm2")
    gelu = (lambda t: F.gelu(t, approximate="tanh")) if "tanh_gelu" in mistakes else F.gelu
    h = O.plain_conv(sd, p + ".mlp.fc1", g2, post=gelu)
    return O.plain_conv(sd, p + ".mlp.fc2", h, post=lambda t: y1 + ls(2) * t)


def evc_block(sd, p, x, mistakes=()):
    """EVCBlock.forward with in == out channels"""
    t = _conv_bn(sd, p + ".conv1", p + ".bn1", x, 3, 1e-5)
    x1 = t if "no_maxpool" in mistakes else F.max_pool2d(t, 3, 1, 1)
    with bn_eps(1e-5):
        a, b = lvc_block(sd, p + ".lvc", x1, mistakes), light_mlp(sd, p + ".l_MLP", x1, mistakes)
    return O.plain_conv(sd, p + ".cnv1", torch.cat((b, a) if "concat_swapped" in mistakes else (a, b), 1))


def cfp_forward(sd, x, mistakes=()):
    """models.cfp.yolox_cfp.YoloBody.forward -> the three raw outputs [n, 5 + nc, H_l, W_l]"""
    p = "backbone"
    f = O.csp_darknet(sd, p + ".backbone", x)                           # base/baseConv.py's eps 1e-3
    feat1, feat2, feat3 = f["dark3"], f["dark4"], f["dark5"]
    with bn_eps(1e-3 if "eps_neck_head_1e-3" in mistakes else 1e-5):
        P5 = O.base_conv(sd, p + ".lateral_conv0", feat3)
        if "evc_before_upsample" in mistakes:
            up = O._up2(evc_block(sd, p + ".evcblock", P5, mistakes))
        else:
            up = evc_block(sd, p + ".evcblock", O._up2(P5), mistakes)
        t = O.csp_layer(sd, p + ".C3_p4", torch.cat((up, feat2), 1), False)
        P4 = O.base_conv(sd, p + ".reduce_conv1", t)
        P3_out = O.csp_layer(sd, p + ".C3_p3", torch.cat((O._up2(P4), feat1), 1), False)
        d = O.any_conv(sd, p + ".bu_conv2", P3_out, 2)
        P4_out = O.csp_layer(sd, p + ".C3_n3", torch.cat((d, P4), 1), False)
        d = O.any_conv(sd, p + ".bu_conv1", P4_out, 2)
        P5_out = O.csp_layer(sd, p + ".C3_n4", torch.cat((d, P5), 1), False)
        return O.yolox_head(sd, "head", (P3_out, P4_out, P5_out))


def run_block(kind, sd, x, mistakes=()):
    fn = {"lvc": lambda: lvc_block(sd, "blk.lvc", x, mistakes), "l_MLP": lambda: light_mlp(sd, "blk.l_MLP", x, mistakes),
          "evc": lambda: evc_block(sd, "blk", x, mistakes)}[kind]
    with torch.no_grad(), bn_eps(1e-5):
        return fn()


def mistake_distance(name):
    """how far the restatement with the planted mistake `name` lands from the record MISTAKES names for it (rel())"""
    where = MISTAKES[name]
    with torch.no_grad():
        if where[0] == "case":
            phi, shape = CASES[where[1]]
            return rel(cfp_forward(weights(phi), case_input(phi, shape), {name}), recorded(phi, shape))
        if where[0] == "encoding":
            rec, C, h, w, n = ENCODING_RECORDS[where[1]]
            sd = block_weights(C)
            got = encoding(block_input(C, h, w, n, key=1), sd["blk.lvc.LVC.3.codewords"], sd["blk.lvc.LVC.3.scale"], {name})
            return rel(got, block_recorded("encoding", rec))
        rec, C, h, w, n = BLOCK_RECORDS[where[2]]
        return rel(run_block(where[1], block_weights(C), block_input(C, h, w, n), {name}), block_recorded(where[1], rec))


# ------------------------------------------------------------------------------------------ glsdet_lvc_encode: regimes
def encode_operands(C, h, w, n, seed, regime):
    """(x [n, C, h, w], codewords [64, C], scale [64]) fp32 for tests/test_lvc_exact.py.
    'uniform': scale = 0, so every weight is exactly 1 / 64; x, c multiples of 1/8 in [-2, 2]: every partial sum of
        A^T X (multiples of 2^-9 below 2^14) and of (sum A) c is exact in fp32 in any order, E is THE exact sum.
    'onehot': codeword k is 8 on the channels j with j % 32 == k % 32 .. see onehot_margin; x_n = c_k(n) + an offset in
        {-1/4, 0, 1/4}; scale = -4: foreign logits lie ONEHOT_MARGIN below the own one, expf gives exactly 0 and the own
        weight exactly 1; all of D's terms are multiples of 1/16 below 2^24 / 16: exact in any order.
    'continuous': x of order 1, codewords of order 0.3, scale in (-1, 0)."""
    rng = np.random.default_rng([seed, C, h * w, n])
    N = h * w
    if regime == "uniform":
        x = rng.integers(-16, 17, (n, C, h, w)) / 8.0
        cw = rng.integers(-16, 17, (NUM_CODES, C)) / 8.0
        sc = np.zeros(NUM_CODES)
    elif regime == "onehot":
        cw = onehot_codewords(C)
        owner = rng.integers(0, NUM_CODES, (n, N))
        off = rng.integers(-1, 2, (n, N, C)) / 4.0
        x = (cw[owner] + off).transpose(0, 2, 1).reshape(n, C, h, w)
        sc = np.full(NUM_CODES, -4.0)
    else:
        x = rng.standard_normal((n, C, h, w))
        cw = 0.3 * rng.standard_normal((NUM_CODES, C))
        sc = -rng.uniform(0.05, 1.0, NUM_CODES)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return f(x), f(cw), f(sc)


def onehot_codewords(C):
    """64 codewords with entries in {0, 8}: codeword k = 8 * (bits of the 6-bit code of k and of its complement, repeated
    over the channels), so that two codewords differ on at least C / 12 >= 2 channels (C >= 32) by 8 each."""
    k = np.arange(NUM_CODES)
    bits = ((k[:, None] >> np.arange(6)[None, :]) & 1)
    pat = np.concatenate([bits, 1 - bits], 1)                           # [64, 12]: any two rows differ in >= 2 places
    return 8.0 * pat[:, np.arange(C) % 12]


ONEHOT_MARGIN = 110.0


def onehot_margin(x, cw, sc):
    """min over pixels of (own logit - best foreign logit), float64: must exceed ONEHOT_MARGIN.  With offsets of at most
    1/4 per channel, own |x - c|^2 <= C / 16 and a foreign one >= 2 (8 - 1/4)^2 per differing pair of channels times
    floor(C / 12) repetitions, at scale -4."""
    B, C = x.shape[:2]
    X = x.double().reshape(B, C, -1).transpose(1, 2)
    D = sc.double() * (X[:, :, None, :] - cw.double()[None, None]).pow(2).sum(3)
    top = D.topk(2, dim=2).values
    return float((top[..., 0] - top[..., 1]).min())


# ------------------------------------------------------------------------------------------------------ a-priori bound
U32 = 2.0 ** -24


def encode_bound(x, cw, sc):
    """Per-element bound [B, 64, C] on |E_fp32 - E_exact| for glsdet_lvc_encode's evaluation (and for the reference's own
    fp32 one), from the exact (float64) quantities.  u = 2^-24, T_nk = sum_j (|x_nj| + |c_kj|)^2, N pixels.
      logits   |x|^2, x.c, |c|^2 are C-term fp32 sums in some order and three more roundings join them:
               |dD_nk| <= |s_k| (C + 3) u T_nk + u |D_nk|          (the definition's sum of squared differences: the same)
               + u |D_nk - max_k D| for the shift; an error of the maximum itself shifts a row as a whole and cancels.
      expf     one ulp of the result (2 u relative) on top of e^dD - 1
      softmax  the 64-term sum (66 u) and the division (u): weights with relative error
               rho_nk <= d_nk + sum_j A_nj d_nj + 70 u,  d = the bound on dD
      E        both products read the SAME rounded weights, so their errors meet as sum_n rho_nk A_nk |x_nc - c_kc|; the two
               N-term accumulations (tiles, then up to 64 slices) add (N + 66) u (sum_n A_nk |x_nc| + S_k |c_kc|) and the
               last fmaf one rounding of the result.
      underflow  a weight below 2^-126 may be flushed to zero (expf, the division, the products): N 2^-125 max |x - c| absolute.
    Second-order terms are covered by the factor 2 on the whole."""
    B, C = x.shape[:2]
    X = x.double().reshape(B, C, -1).transpose(1, 2)
    c, s = cw.double(), sc.double()
    N = X.shape[1]
    T = X.pow(2).sum(2, keepdim=True) + 2.0 * X.abs() @ c.abs().t() + c.pow(2).sum(1)
    D = s * ((X.pow(2).sum(2, keepdim=True) - 2.0 * X @ c.t()) + c.pow(2).sum(1))
    A = torch.softmax(D, 2)
    d = s.abs() * (C + 3) * U32 * T + U32 * D.abs() + U32 * (D - D.max(2, keepdim=True).values).abs()
    rho = d + (A * d).sum(2, keepdim=True) + 70 * U32                   # [B, N, 64]
    absdiff = (X[:, :, None, :] - c[None, None]).abs()                  # [B, N, 64, C]
    first = ((rho * A)[..., None] * absdiff).sum(1)
    second = (N + 66) * U32 * (A.transpose(1, 2) @ X.abs() + A.sum(1)[:, :, None] * c.abs())
    E = A.transpose(1, 2) @ X - A.sum(1)[:, :, None] * c
    return 2.0 * (first + second + U32 * E.abs()) + N * 2.0 ** -125 * float(absdiff.max()), E


# ------------------------------------------------------------------------------- gate / fuse in their documented order
def gate_fp32(E, a, b, W, bias):
    """glsdet_lvc_gate's order (include/glsdet_hip.h) in numpy float32; on dyadic data every step is exact, so fmaf and
    multiply-add agree.  -> (v before the sigmoid [n, C] fp32, sigmoid(v) in float64)"""
    E, a, b, W, bias = (np.asarray(t, np.float32) for t in (E, a, b, W, bias))
    n, K, C = E.shape
    m = np.zeros((n, C), np.float32)
    for k in range(K):
        m = m + np.maximum(a[k] * E[:, k, :] + b[k], np.float32(0))
    en = m * np.float32(1.0 / K)
    v = np.broadcast_to(bias, (n, C)).astype(np.float32).copy()
    for c in range(C):
        v = v + W[None, :, c] * en[:, c:c + 1]
    return v, 1.0 / (1.0 + np.exp(-v.astype(np.float64)))
