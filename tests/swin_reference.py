"""Float64 restatement, from the definition, of the reference's Swin trunk (ufp/mmdet/models/backbones/swin.py and
PatchEmbed / PatchMerging of ufp/mmdet/models/utils/transformer.py), the a-priori error bounds of the kernels in
csrc/swin.hip, and the operand generators of tests/test_swin_exact.py.  tests/test_swin_reference.py holds every function
here to the outputs tests/golden/swin_golden.npz records of the reference's own modules.

Layout: activations are [n, H, W, C] (the reference's [B, L, C] with L = H * W unrolled); weights carry mmdet's names.
`mis` names ONE planted misreading (tests/test_swin_reference.py shows a fixture that sees each); `rnd` is the rounding
applied at the store points of the kernels (identity in float64; through fp16 for the f16 emulation).

The window attention follows the reference's own steps -- pad, roll, img_mask by slices, partition, softmax, reverse, roll
back, crop -- while the kernel computes every token from coordinates: the two share no index arithmetic."""
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from glsdet_amd.synth import synth_input, synth_tensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24                       # unit roundoff of fp32
ONEHOT_MARGIN = 110.0                  # expf(-x) is exactly 0 in fp32 for x > 103.98
MISREADINGS = ("pad_zero", "pad_masked", "mask_inf", "regions_unpadded", "regions_unshifted", "roll_sign", "no_flip",
               "scale_after_bias", "unfold_khkwc", "merge_pad_after_norm", "skip_norm_i", "ln_axis")
TINY = dict(embed_dims=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), window_size=7)
_G = {}


def golden():
    if not _G:
        g = np.load(os.path.join(ROOT, "tests", "golden", "swin_golden.npz"))
        _G.update({k: g[k] for k in g.files})
    return _G


def meta(tag):
    return json.loads(golden()["block/%s/meta" % tag].tobytes().decode())


def weights(tag, dtype=torch.float64):
    m = meta(tag)
    return {k: torch.from_numpy(synth_tensor(k, tuple(s), m["seed"])).to(torch.int64 if k.endswith("_index") else dtype)
            for k, s in m["shapes"].items()}


def block_input(tag):
    m = meta(tag)
    return synth_input(tuple(m["in_shape"]), m["seed"] + 100)


def ident(t):
    return t


def f16_round(t):
    return t.to(torch.float16).to(t.dtype)


# ------------------------------------------------------------------------------------------------ the definition
def rel_index(ws, flip=True):
    """relative_position_index as swin.py:64-68 builds it: double_step_seq(2 ws - 1, ws, 1, ws), + its transpose, flip(1)"""
    seq = (torch.arange(0, (2 * ws - 1) * ws, 2 * ws - 1)[:, None] + torch.arange(0, ws)[None, :]).reshape(1, -1)
    idx = seq + seq.T
    return idx.flip(1).contiguous() if flip else idx


def layernorm(x, g, b, eps=1e-5, mis=None):
    if mis == "ln_axis":                          # over the tokens of an image instead of the channels
        n, H, W, C = x.shape
        t = x.reshape(n, H * W, C)
        mu, var = t.mean(1, keepdim=True), t.var(1, unbiased=False, keepdim=True)
        return (((t - mu) / torch.sqrt(var + eps)) * g + b).reshape(n, H, W, C)
    mu, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def _partition(t, ws):
    n, Hp, Wp, C = t.shape
    return t.reshape(n, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)


def _reverse(t, ws, n, Hp, Wp):
    return t.reshape(n, Hp // ws, Wp // ws, ws, ws, -1).permute(0, 1, 3, 2, 4, 5).reshape(n, Hp, Wp, -1)


def _regions(Hr, Wr, ws, shift):
    m = torch.zeros(Hr, Wr, dtype=torch.float64)
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            m[hs, wsl] = cnt
            cnt += 1
    return m


def window_attention(qkv, table, qkv_bias, heads, ws, shift, scale=None, mis=None, extras=None):
    """ShiftWindowMSA.forward + WindowMSA.forward between the qkv and the proj linear: qkv [n, H, W, 3C] (the linear's output
    on the unpadded map) -> [n, H, W, C].  extras (a dict) receives 'margin' [n, H, W, heads], the distance of each real
    query row's largest logit from its second largest, 'padded_winner' (1 where that largest logit is a padded token's)
    and 'bound', the a-priori error bound of the kernel (below)."""
    n, H, W, C3 = qkv.shape
    C = C3 // 3
    hd = C // heads
    scale = hd ** -0.5 if scale is None else scale
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    fillv = qkv_bias if (qkv_bias is not None and mis != "pad_zero") else torch.zeros(C3, dtype=qkv.dtype)
    full = fillv.to(qkv.dtype).expand(n, Hp, Wp, C3).clone()
    full[:, :H, :W] = qkv
    real = torch.zeros(1, Hp, Wp, 1, dtype=torch.float64)
    real[:, :H, :W] = 1
    mask = None
    if shift > 0:
        by = shift if mis == "roll_sign" else -shift
        full, real = torch.roll(full, (by, by), (1, 2)), torch.roll(real, (by, by), (1, 2))
        if mis == "regions_unpadded":             # the slices of swin.py:200-205 taken on H x W, the pad rows joining the last
            img = _regions(H, W, ws, shift)[torch.arange(Hp).clamp(max=H - 1)][:, torch.arange(Wp).clamp(max=W - 1)]
        else:
            img = _regions(Hp, Wp, ws, shift)
        if mis == "regions_unshifted":            # the region map rolled along with the image
            img = torch.roll(img, (-shift, -shift), (0, 1))
        mw = _partition(img[None, :, :, None], ws)[..., 0]                    # [nW, N]
        diff = mw[:, None, :] - mw[:, :, None]
        mask = torch.where(diff != 0, torch.tensor(-math.inf if mis == "mask_inf" else -100.0, dtype=torch.float64),
                           torch.tensor(0.0, dtype=torch.float64))
    xw = _partition(full, ws)                                                   # [B, N, 3C]
    rw = _partition(real.expand(n, Hp, Wp, 1), ws)[..., 0]                     # [B, N] 1 = a token of the map
    B, N, _ = xw.shape
    q, k, v = xw.reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    bias = table[rel_index(ws, flip=mis != "no_flip").reshape(-1)].reshape(N, N, heads).permute(2, 0, 1)
    if mis == "scale_after_bias":
        attn = (q @ k.transpose(-2, -1) + bias[None]) * scale
    else:
        attn = (q * scale) @ k.transpose(-2, -1) + bias[None]
    if mask is not None:
        nW = mask.shape[0]
        attn = (attn.reshape(B // nW, nW, heads, N, N) + mask[None, :, None]).reshape(B, heads, N, N)
    if mis == "pad_masked":
        attn = attn + torch.where(rw > 0, 0.0, -math.inf)[:, None, None, :]
    p = torch.softmax(attn, -1)
    out = (p @ v).transpose(1, 2).reshape(B, N, C)

    def back(t):
        t = _reverse(t, ws, n, Hp, Wp)
        if shift > 0:
            by_ = -shift if mis == "roll_sign" else shift
            t = torch.roll(t, (by_, by_), (1, 2))
        return t[:, :H, :W].contiguous()

    if extras is not None:
        top = attn.topk(2, -1).values
        extras["margin"] = back((top[..., 0] - top[..., 1]).transpose(1, 2))   # [B, N, heads] -> the map
        # 1 where the row's largest logit belongs to a padded token (a key outside the map), per real query row and head
        won = torch.gather(rw[:, None, None, :].expand(B, heads, N, N), -1, attn.argmax(-1, keepdim=True))[..., 0]
        extras["padded_winner"] = back((1 - won).transpose(1, 2))
        # ---- the a-priori bound of glsdet_window_attention, per output element (u = 2^-24):
        #   q~ = fl(q scale), S^ an fmaf chain of 32 products, two more adds (bias, mask):
        #       |S^ - S| <= E = u (34 A + 2 (|logit| + 2 |bias| + 2 |mask|)),  A = sum_d |q~_d| |k_d|
        #       (|q~ . k| and |q~ . k + bias| are each at most |logit| + |bias| + |mask|)
        #   x = S^ - max^ (one rounding, |x| <= R, the spread of the row), expf within 2 ulp, the row sum of N terms and the
        #   division: the weight p_j carries a relative error of at most
        #       T = 2 (2 E + u R + 2 u) + (N + 1) u          (E, R the row's maxima; the shift by max^ cancels in the ratio)
        #   O = the fmaf chain of N (+ 1) terms p_j v_j:   |O^ - O| <= (T + (N + 2) u) sum_j p_j |v_j|
        # times 1.05 for the second-order terms, plus the rounding to the storage type applied by the caller.
        A = (q * scale).abs() @ k.abs().transpose(-2, -1)
        msk = 0.0 if mask is None else mask.abs()[None, :, None].expand(B // mask.shape[0], -1, heads, -1, -1).reshape(B, heads, N, N)
        fin = torch.where(torch.isfinite(attn), attn, torch.zeros_like(attn))
        E = U32 * (34 * A + 2 * (fin.abs() + 2 * bias.abs()[None] + 2 * msk))
        R = fin.max(-1).values - fin.min(-1).values
        T = 2 * (2 * E.max(-1).values + U32 * R + 2 * U32) + (N + 1) * U32
        bnd = 1.05 * (T + (N + 2) * U32)[..., None] * (p @ v.abs())
        extras["bound"] = back(bnd.transpose(1, 2).reshape(B, N, C))
    return back(out)


def patch_merge(x, mis=None):
    """AdaptivePadding('corner') + nn.Unfold(2, stride 2): [n, H, W, C] -> [n, ceil(H/2), ceil(W/2), 4C], channel 4 c + 2 kh + kw"""
    n, H, W, C = x.shape
    t = x.permute(0, 3, 1, 2)
    t = F.pad(t, [0, W % 2, 0, H % 2])
    Ho, Wo = t.shape[2] // 2, t.shape[3] // 2
    u = F.unfold(t, 2, stride=2)                                                # [n, 4C, Ho * Wo], channel-major
    if mis == "unfold_khkwc":
        u = u.reshape(n, C, 4, Ho * Wo).permute(0, 2, 1, 3).reshape(n, 4 * C, Ho * Wo)
    return u.transpose(1, 2).reshape(n, Ho, Wo, 4 * C)


def linear(x, w, b=None, rnd=ident):
    y = x @ rnd(w).T
    return rnd(y if b is None else y + b)


def msa(x, wts, p, heads, ws, shift, scale=None, mis=None, rnd=ident, rnd_out=None):
    """ShiftWindowMSA on an [n, H, W, C] map; p = the module's prefix ('...attn.')"""
    bq = wts.get(p + "w_msa.qkv.bias")
    qkv = linear(x, wts[p + "w_msa.qkv.weight"], bq, rnd)
    a = rnd(window_attention(qkv, wts[p + "w_msa.relative_position_bias_table"], None if bq is None else rnd(bq), heads, ws,
                             shift, scale, mis))
    return (rnd_out or rnd)(a @ rnd(wts[p + "w_msa.proj.weight"]).T + wts[p + "w_msa.proj.bias"])


def merging(x, wts, p, mis=None, rnd=ident):
    """PatchMerging: pad + unfold, LayerNorm over 4C (the padded zeros take part), reduction (no bias)"""
    u = patch_merge(x, mis)                       # a permutation of the stream: no rounding of its own
    y = layernorm(u, wts[p + "norm.weight"], wts[p + "norm.bias"])
    if mis == "merge_pad_after_norm":             # the zero fill applied to the normalised tensor instead
        live = patch_merge(torch.ones_like(x), mis)
        y = y * live
    return linear(rnd(y), wts[p + "reduction.weight"], None, rnd)


def swin_block(x, wts, p, heads, ws, shift, scale=None, mis=None, rnd=ident, rnd_res=ident):
    """SwinBlock.forward (swin.py:357-377); rnd_res: the rounding of the residual stream"""
    y = rnd(layernorm(x, wts[p + "norm1.weight"], wts[p + "norm1.bias"], mis=mis))
    x = rnd_res(x + msa(y, wts, p + "attn.", heads, ws, shift, scale, mis, rnd, rnd_out=ident))
    y = rnd(layernorm(x, wts[p + "norm2.weight"], wts[p + "norm2.bias"], mis=mis))
    h = rnd(F.gelu(y @ rnd(wts[p + "ffn.layers.0.0.weight"]).T + wts[p + "ffn.layers.0.0.bias"]))
    return rnd_res(x + (h @ rnd(wts[p + "ffn.layers.1.weight"]).T + wts[p + "ffn.layers.1.bias"]))


def trunk(img, wts, embed_dims=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), window_size=7, out_indices=(0, 1, 2, 3),
          patch_norm=True, qk_scale=None, mis=None, rnd=ident, rnd_res=ident, p="backbone."):
    """SwinTransformer.forward (swin.py:744-762): NCHW image -> the NCHW maps after norm{i}"""
    n, _, H, W = img.shape
    t = F.pad(rnd(img), [0, (-W) % 4, 0, (-H) % 4])
    x = F.conv2d(t, rnd(wts[p + "patch_embed.projection.weight"]), wts[p + "patch_embed.projection.bias"], stride=4)
    x = rnd_res(x.permute(0, 2, 3, 1))
    if patch_norm:
        x = rnd_res(layernorm(x, wts[p + "patch_embed.norm.weight"], wts[p + "patch_embed.norm.bias"], mis=mis))
    outs = []
    for i, depth in enumerate(depths):
        for j in range(depth):
            x = swin_block(x, wts, "%sstages.%d.blocks.%d." % (p, i, j), num_heads[i], window_size,
                           window_size // 2 if j % 2 else 0, qk_scale, mis, rnd, rnd_res)
        if i in out_indices:
            o = x if mis == "skip_norm_i" else rnd(layernorm(x, wts["%snorm%d.weight" % (p, i)], wts["%snorm%d.bias" % (p, i)], mis=mis))
            outs.append(o.permute(0, 3, 1, 2).contiguous())
        if i < len(depths) - 1:
            x = rnd_res(merging(x, wts, "%sstages.%d.downsample." % (p, i), mis, rnd))
    return outs


def state_dict_shapes(embed_dims=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), window_size=7, mlp_ratio=4,
                      out_indices=(0, 1, 2, 3), patch_norm=True, qkv_bias=True, in_channels=3):
    """the names and shapes of SwinTransformer.state_dict(), in the order the modules register them"""
    from glsdet_amd.arch import swin_state_dict_shapes
    return swin_state_dict_shapes(embed_dims, depths, num_heads, window_size, mlp_ratio, out_indices, patch_norm, qkv_bias,
                                  in_channels)


# ------------------------------------------------------------------------------------------------ LayerNorm bound
def layernorm_bound(x, g, b, eps, out_f16=False):
    """A-priori bound of glsdet_layernorm per element, x [.., C] float64 holding the kernel's (representable) input.
    k = ceil(C / 256) + 9 bounds the roundings any element meets on its way into a sum (its lane's chain, the two adds inside
    a 4-vector, six butterfly steps, the division), a = max |x| of the row:
        |mean^ - mean| <= dm = k u a
        d^ = fl(x - mean^):  |d^ - d| <= dd = dm + u |d|
        var^ = the same sum over d^ d^:  |var^ - var| <= dv = 2 sqrt(var) dm + dm^2 + (k + 5) u var
        rstd^ = 1 / sqrtf(var^ + eps):  relative error <= rr = dv / (2 (var + eps)) + 3 u
        y^ = fl(fl(fl(d^ rstd^) gamma) + beta):  |y^ - y| <= |gamma| rstd (dd + |d| (rr + 2 u)) + u |y|
    times 1.05 for the second-order terms; an fp16 output adds half an ulp of the result (2^-11 |y| + 2^-25)."""
    C = x.shape[-1]
    k = -(-C // 256) + 9
    a = x.abs().max(-1, keepdim=True).values
    mu, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    d = x - mu
    rstd = 1 / torch.sqrt(var + eps)
    y = d * rstd * g + b
    dm = k * U32 * a
    dd = dm + U32 * d.abs()
    dv = 2 * torch.sqrt(var) * dm + dm * dm + (k + 5) * U32 * var
    rr = dv / (2 * (var + eps)) + 3 * U32
    bound = 1.05 * (g.abs() * rstd * (dd + d.abs() * (rr + 2 * U32)) + U32 * y.abs())
    if out_f16:
        bound = bound + 2.0 ** -11 * y.abs() + 2.0 ** -25
    return bound, y


# ------------------------------------------------------------------------------------------------ operands of the exact tests
def attention_operands(n, H, W, heads, ws, regime, seed):
    """-> (qkv [n, H, W, 3C] float64, table [(2 ws - 1)^2, heads], qkv_bias [3C]), every value representable in fp16.
    'onehot': the table holds 512 * (a permutation of the offsets) per head, so for a fixed query every key -- padded tokens
        included: they share k = the bias but not their offset -- has its own bias, 512 apart; q in {-2..2}, k in {-1, 0, 1}:
        |q~ . k| <= 64 * 32^-0.5 < 11.4, and the mask costs at most 100: the row's winner leads by more than 512 - 100 - 23 >
        ONEHOT_MARGIN (asserted by the caller from extras['margin']).  fp32 expf of anything below -103.98 is exactly 0, so the
        weights are exactly one-hot and the output is the winner's v, bit for bit.  (A row that ONLY the mask decides has a lead
        of at most 100: no such row can be one-hot in fp32, they belong to the 'regions' regime.)
    'regions': q = 0 on every token of the map and a zero table: the logits of a row are 0 inside the query's mask region and
        -100 outside, so the weights are 1 / count over the region, padded tokens included
    'continuous': normal q, k, v of order 1, a normal table of order 0.5"""
    rng = np.random.default_rng([seed, n, H, W, heads, ws, len(regime)])
    C = 32 * heads
    span = (2 * ws - 1) ** 2
    if regime == "continuous":
        qkv = np.round(rng.standard_normal((n, H, W, 3 * C)) * 256) / 256
        table = 0.5 * rng.standard_normal((span, heads))
        bias = np.round(0.5 * rng.standard_normal(3 * C) * 256) / 256
    else:
        q = rng.integers(-2, 3, (n, H, W, C)).astype(np.float64)
        k = rng.integers(-1, 2, (n, H, W, C)).astype(np.float64)
        v = rng.choice(np.concatenate([np.arange(-32, 0), np.arange(1, 33)]) / 8.0, (n, H, W, C))
        bias = np.concatenate([rng.integers(-2, 3, C), rng.integers(-1, 2, C), rng.integers(-16, 17, C) / 4.0]).astype(np.float64)
        if regime == "onehot":
            table = np.stack([512.0 * rng.permutation(span) for _ in range(heads)], 1)
        else:
            q[:] = 0
            table = np.zeros((span, heads))
        qkv = np.concatenate([q, k, v], -1)
    f = lambda t: torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64))
    return f(qkv), f(table.astype(np.float32)), f(bias)


def regions_bound(v_absmax, N, out_f16=False):
    """the 'regions' regime: p = fl(1 / count) (half an ulp; the row sum is the exact count -- the weights of the other
    regions are e^-100, below 2^-144), then a chain of at most N + 1 fmaf roundings of partial sums no larger than max |v|:
    (N + 2) roundings of half an ulp of max |v| each, i.e. <= (N + 2) u max |v| -- at most 66 u max |v| for a full window;
    the masked keys add less than N * 2^-144 max |v|"""
    b = (N + 2) * U32 * v_absmax + 2.0 ** -120
    return b + (2.0 ** -11 * v_absmax if out_f16 else 0.0)
