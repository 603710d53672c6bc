#!/usr/bin/env python3
"""Measurement of the Swin trunk (run by hand on an MI355X; bench.py is the gated benchmark and is not involved):

  Swin-T + FPN + GFLHead at 8 x 800 x 1344, f16, from a captured plan: ms per batch and img/s over repeated windows, and the
  share of the plan's time per kernel family (attention, LayerNorm, linears of the trunk, merge; neck + head as the rest)
  from an eager replay with an event pair around every op
against
  (a) a torch restatement of the same trunk, run eagerly on the same GPU in fp16 (pad / roll / partition / bmm + softmax +
      bmm / F.layer_norm / F.linear), and the bmm + softmax + bmm of its windows alone against the window-attention launches;
  (b) the ResNet-50 and ResNeXt-101-32x4d detectors (same neck and head) from their captured plans.

Weights are synthetic (glsdet_amd.synth): times do not depend on them.  Prints one JSON object.

    python tools/swin_bench.py [--batch 8] [--height 800] [--width 1344] [--windows 5] [--iters 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWIN_T = dict(embed_dims=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), window_size=7)


def windows_of(fn, windows, iters):
    """-> ms per call of fn() over `windows` windows of `iters` calls, each ended by a device synchronise"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    return out


def plan_times(det, n, H, W, windows, iters):
    c = det.compile(n, H, W, use_graph=True)
    x = torch.randn(n, 3, H, W, device="cuda")
    det.run(c, x)
    torch.cuda.synchronize()
    return c, windows_of(lambda: det.run(c), windows, iters)


def family(name):
    for key, fam in (("window_attention", "attention"), ("layernorm", "layernorm"), ("patch_merge", "merge")):
        if name.startswith(key):
            return fam
    return "conv"


# ---- (a) the same trunk in eager torch, fp16
def torch_attention(qkv, table_bias, mask, heads, ws, shift):
    """qkv [n, Hp, Wp, 3C] (already padded) -> [n, Hp, Wp, C]"""
    n, Hp, Wp, C3 = qkv.shape
    C = C3 // 3
    if shift:
        qkv = torch.roll(qkv, (-shift, -shift), (1, 2))
    xw = qkv.reshape(n, Hp // ws, ws, Wp // ws, ws, C3).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, 3, heads, C // heads)
    q, k, v = xw.permute(2, 0, 3, 1, 4)
    attn = (q * (C // heads) ** -0.5) @ k.transpose(-2, -1) + table_bias
    if mask is not None:
        nW = mask.shape[0]
        attn = (attn.reshape(-1, nW, heads, ws * ws, ws * ws) + mask[None, :, None]).reshape(-1, heads, ws * ws, ws * ws)
    o = (torch.softmax(attn, -1) @ v).transpose(1, 2).reshape(n, Hp // ws, Wp // ws, ws, ws, C)
    o = o.permute(0, 1, 3, 2, 4, 5).reshape(n, Hp, Wp, C)
    return torch.roll(o, (shift, shift), (1, 2)) if shift else o


def torch_trunk(sd, img, cfg, core_log=None):
    """the trunk on NHWC tensors of img's dtype; core_log collects (windows, heads, N, head_dim) of every attention"""
    from glsdet_amd.synth import synth_tensor
    p = "backbone."
    ws = cfg["window_size"]
    idx = torch.from_numpy(synth_tensor("relative_position_index", (ws * ws, ws * ws), 0)).to(img.device).reshape(-1)
    x = F.conv2d(img, sd[p + "patch_embed.projection.weight"], sd[p + "patch_embed.projection.bias"], stride=4).permute(0, 2, 3, 1)
    x = F.layer_norm(x, x.shape[-1:], sd[p + "patch_embed.norm.weight"], sd[p + "patch_embed.norm.bias"])
    outs = []
    for i, depth in enumerate(cfg["depths"]):
        heads = cfg["num_heads"][i]
        n, H, W, C = x.shape
        Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
        for j in range(depth):
            q = "%sstages.%d.blocks.%d." % (p, i, j)
            shift = ws // 2 if j % 2 else 0
            y = F.layer_norm(x, (C,), sd[q + "norm1.weight"], sd[q + "norm1.bias"])
            y = F.pad(y, (0, 0, 0, Wp - W, 0, Hp - H))
            qkv = F.linear(y, sd[q + "attn.w_msa.qkv.weight"], sd[q + "attn.w_msa.qkv.bias"])
            tb = sd[q + "attn.w_msa.relative_position_bias_table"][idx].reshape(ws * ws, ws * ws, heads).permute(2, 0, 1)
            mask = None
            if shift:
                m = torch.zeros(Hp, Wp, device=x.device)
                for a, hs in enumerate((slice(0, -ws), slice(-ws, -shift), slice(-shift, None))):
                    for b, wsl in enumerate((slice(0, -ws), slice(-ws, -shift), slice(-shift, None))):
                        m[hs, wsl] = 3 * a + b
                mw = m.reshape(Hp // ws, ws, Wp // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)
                mask = ((mw[:, None, :] - mw[:, :, None]) != 0).to(x.dtype) * -100.0
            if core_log is not None:
                core_log.append((n * (Hp // ws) * (Wp // ws), heads, ws * ws, C // heads))
            o = torch_attention(qkv, tb, mask, heads, ws, shift)[:, :H, :W]
            x = x + F.linear(o, sd[q + "attn.w_msa.proj.weight"], sd[q + "attn.w_msa.proj.bias"])
            y = F.layer_norm(x, (C,), sd[q + "norm2.weight"], sd[q + "norm2.bias"])
            y = F.gelu(F.linear(y, sd[q + "ffn.layers.0.0.weight"], sd[q + "ffn.layers.0.0.bias"]))
            x = x + F.linear(y, sd[q + "ffn.layers.1.weight"], sd[q + "ffn.layers.1.bias"])
        if i in cfg["out_indices"]:
            outs.append(F.layer_norm(x, (C,), sd["%snorm%d.weight" % (p, i)], sd["%snorm%d.bias" % (p, i)]))
        if i < len(cfg["depths"]) - 1:
            d = "%sstages.%d.downsample." % (p, i)
            t = F.pad(x.permute(0, 3, 1, 2), (0, W % 2, 0, H % 2))
            u = F.unfold(t, 2, stride=2).transpose(1, 2).reshape(n, (H + 1) // 2, (W + 1) // 2, 4 * C)
            u = F.layer_norm(u, (4 * C,), sd[d + "norm.weight"], sd[d + "norm.bias"])
            x = F.linear(u, sd[d + "reduction.weight"])
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1344)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("swin_bench needs an MI355X: a time measured elsewhere says nothing")
    from glsdet_amd.arch import resdet_state_dict_shapes, swindet_state_dict_shapes
    from glsdet_amd.resdet import HipGflDetector
    from glsdet_amd.synth import synth_state_dict
    n, H, W = a.batch, a.height, a.width
    res = {"shape": [n, 3, H, W], "dtype": "f16", "windows": a.windows, "iters": a.iters}
    cfg = dict(SWIN_T, out_indices=(1, 2, 3))
    sd = synth_state_dict(swindet_state_dict_shapes("gfl", **cfg), 0)
    det = HipGflDetector("gfl", sd, dtype="f16", autotune=True, backbone="swin", start_level=0, **cfg)
    c, ms = plan_times(det, n, H, W, a.windows, a.iters)
    res["swin_t"] = {"ms_per_batch": ms, "img_per_s": n * 1e3 / float(np.median(ms))}
    per_op = c.plan.run_timed(reps=3)
    fam = {}
    trunk_ops = max(i for i, o in enumerate(c.plan.ops()) if family(o["name"]) != "conv") + 1      # up to the last norm{i}
    for i, (o, t) in enumerate(zip(c.plan.ops(), per_op)):
        f = family(o["name"])
        f = "linears" if (f == "conv" and i < trunk_ops) else ("neck+head" if f == "conv" else f)
        fam[f] = fam.get(f, 0.0) + float(t)
    res["swin_t"]["ms_by_family_eager_timed"] = fam
    res["swin_t"]["attention_launches"] = sum(1 for o in c.plan.ops() if family(o["name"]) == "attention")
    # (a) torch eager, fp16
    tsd = {k: v.cuda().half() if v.is_floating_point() else v.cuda() for k, v in sd.items() if k.startswith("backbone.")}
    img = torch.randn(n, 3, H, W, device="cuda").half()
    log = []
    with torch.no_grad():
        torch_trunk(tsd, img, cfg, log)
        res["torch_trunk_fp16_eager"] = {"ms_per_batch": windows_of(lambda: torch_trunk(tsd, img, cfg), a.windows, max(2, a.iters // 3))}
        core = 0.0
        for (B, heads, N, hd) in log:                   # bmm + softmax + bmm of the windows of one attention launch
            q = torch.randn(B, heads, N, hd, device="cuda").half()
            core += float(np.median(windows_of(lambda: torch.softmax(q @ q.transpose(-2, -1), -1) @ q, 3, 5)))
        res["torch_trunk_fp16_eager"]["bmm_softmax_bmm_ms_all_blocks"] = core
    # (b) the convolutional detectors of the same neck and head
    for name, kw in (("resnet50", {}), ("resnext101_32x4d", dict(depth=101, groups=32, base_width=4))):
        rsd = synth_state_dict(resdet_state_dict_shapes("gfl", **kw), 0)
        d = HipGflDetector("gfl", rsd, dtype="f16", autotune=True, **kw)
        _, t = plan_times(d, n, H, W, a.windows, a.iters)
        res[name] = {"ms_per_batch": t, "img_per_s": n * 1e3 / float(np.median(t))}
        del d
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
