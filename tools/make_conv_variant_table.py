"""Records tests/golden/conv_variant_table.json: which kernel every tile_hint selects.

For a fixed list of small problems and a fixed list of hints, each conv entry point is RECORDED into a plan (never
launched: recording validates on the host and stores the op, so this needs no GPU and the made-up, aligned operand
addresses below are never dereferenced) and rows() keeps either the op's name (glsdet_plan_op_info) or "REFUSED" plus
the error text.  The fixture groups them per case, {"entry case": {op name or "REFUSED": [hints]}}.  The exact-arithmetic tests pin what every variant computes; this pins WHICH variant a hint
selects (include/glsdet_hip.h: the table at glsdet_conv_desc.tile_hint).

    python tools/make_conv_variant_table.py [out.json]      # rewrites the fixture from the current build

tests/test_conv_variants.py regenerates the rows and compares them with the fixture row by row."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "conv_variant_table.json")

GEMM_HINTS = list(range(16, 32))
GEO_HINTS = [(g << 8) | h for g in (1, 2) for h in (8, 9, 10, 11, 13)]
# tests/test_hip_fuzz.py::HINTS (the test checks that none is missing here) ...
FUZZ_HINTS = [0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13] + GEMM_HINTS + GEO_HINTS + [
    (128 << 16) | 128, (64 << 16) | 128, (64 << 16) | 64, (32 << 16) | 128, (64 << 16) | 64 | 0x8000,
    (128 << 16) | 128 | 0x8000, (128 << 16), (128 << 16) | 0x8000]
# ... the retired 6 / 7, and values the header does not document
UNDOCUMENTED = [14, 15, 32, 0x30a, (16 << 16) | 64]
HINTS = FUZZ_HINTS + [6, 7, 0x10d] + UNDOCUMENTED
HINTS = sorted(set(HINTS), key=HINTS.index)

F16, F32 = 0, 1
SKIP_Y = 1
# name: (x dtype, y dtype, k, stride, cin, cout, n, h, w, residual)
PROBLEMS = {
    "f16_3x3_c64_o64": (F16, F16, 3, 1, 64, 64, 2, 20, 30, False),
    "f16_3x3_c64_o136_res": (F16, F16, 3, 1, 64, 136, 1, 20, 30, True),
    "f16_3x3_c64_o128_ragged": (F16, F16, 3, 1, 64, 128, 1, 13, 21, False),      # 8 x 16 tiles waste > 30 %: auto leaves the halo kernel
    "f16_3x3_c24_o32": (F16, F16, 3, 1, 24, 32, 1, 20, 30, False),
    "f32_3x3_c32_o136": (F32, F32, 3, 1, 32, 136, 1, 20, 30, False),
    "f16_5x5_c64_o128": (F16, F16, 5, 1, 64, 128, 1, 20, 30, False),
    "f16_7x7_c64_o72": (F16, F16, 7, 1, 64, 72, 1, 20, 30, False),
    "f16_3x3s2_c64_o128": (F16, F16, 3, 2, 64, 128, 2, 40, 60, False),
    "f32_3x3s2_c32_o64_res": (F32, F32, 3, 2, 32, 64, 1, 40, 60, True),
    "f16_1x1_c64_o256": (F16, F16, 1, 1, 64, 256, 2, 20, 30, False),             # Cin = one whole 128-byte K step
    "f16_1x1_c72_o24": (F16, F16, 1, 1, 72, 24, 1, 20, 30, False),              # ... a partial one
    "f32_1x1_c32_o64_res": (F32, F32, 1, 1, 32, 64, 1, 20, 30, True),
    "f32_1x1_c40_o136": (F32, F32, 1, 1, 40, 136, 1, 20, 30, False),
    "f16_f32_1x1_c256_o16": (F16, F32, 1, 1, 256, 16, 2, 20, 30, False),         # predictor: fp16 operands, fp32 logits
}
# conv2d_chain: (problem, c0, cin2, cout2, flags)
CHAINS = {
    "f16_3x3_c64_o64+all32": ("f16_3x3_c64_o64", 0, 64, 32, 0),
    "f16_3x3_c64_o64+all32_skipy": ("f16_3x3_c64_o64", 0, 64, 32, SKIP_Y),
    "f16_3x3_c64_o136_res+hi64": ("f16_3x3_c64_o136_res", 64, 64, 64, 0),
    "f32_3x3_c32_o136+lo32": ("f32_3x3_c32_o136", 0, 32, 128, 0),
    "f16_1x1_c64_o256+mid": ("f16_1x1_c64_o256", 128, 64, 64, 0),
    "f16_3x3s2_c64_o128+all_skipy": ("f16_3x3s2_c64_o128", 0, 128, 64, SKIP_Y),
}
# conv2d_multi: (problem, output extents (h, w) of the problems); 4 = grouped, 9 = batched (one geometry)
MULTIS = {
    "4x f16_3x3_c64_o64": ("f16_3x3_c64_o64", [(13, 21), (13, 21), (12, 21), (13, 20)]),
    "4x f32_3x3_c32_o136": ("f32_3x3_c32_o136", [(13, 21), (13, 21), (12, 21), (13, 20)]),
    "4x f16_3x3s2_c64_o128": ("f16_3x3s2_c64_o128", [(26, 42), (26, 42), (24, 42), (26, 40)]),
    "4x f16_1x1_c72_o24": ("f16_1x1_c72_o24", [(13, 21), (7, 9), (13, 21), (7, 9)]),
    "9x f16_1x1_c64_o256": ("f16_1x1_c64_o256", [(13, 21)] * 9),
    "9x f32_1x1_c32_o64_res": ("f32_1x1_c32_o64_res", [(13, 21)] * 9),
}
# conv2d_gnstats: (problem, groups)
GNSTATS = {
    "f16_3x3_c64_o64 g4": ("f16_3x3_c64_o64", 4),
    "f32_3x3_c32_o136 g17": ("f32_3x3_c32_o136", 17),
    "f16_3x3s2_c64_o128 g8": ("f16_3x3s2_c64_o128", 8),
}


def _view(_lib, n, h, w, c, dtype, base):
    es = 2 if dtype == F16 else 4
    v = _lib.View()
    v.base, v.n, v.h, v.w, v.c, v.dtype = base, n, h, w, c, dtype
    v.sw, v.sh, v.sn = c, w * c, h * w * c
    v.alloc_lo, v.alloc_hi = base, base + n * h * w * c * es
    return v


def _desc(_lib, d, problem, hint, slot=0, out_hw=None):
    """fill the descriptor `d` for `problem`; `slot` moves the made-up addresses, out_hw overrides the output extent"""
    xdt, ydt, k, stride, cin, cout, n, h, w, res = PROBLEMS[problem]
    if out_hw is not None:
        h, w = (out_hw[0] - 1) * stride + 1, (out_hw[1] - 1) * stride + 1
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    base = 0x10000000 + slot * 0x01000000
    d.x = _view(_lib, n, h, w, cin, xdt, base)
    d.y = _view(_lib, n, ho, wo, cout, ydt, base + 0x20000000)
    if res:
        d.res = _view(_lib, n, ho, wo, cout, ydt, base + 0x40000000)
    d.w, d.scale, d.bias = base + 0x60000000, base + 0x60800000, base + 0x60900000
    d.R = d.S = k
    d.stride, d.pad, d.act, d.tile_hint = stride, pad, 1, hint
    return d


def _recorded(_lib, lib, call):
    """run `call` while recording a plan: the op's name, or REFUSED + the error text"""
    plan = lib.glsdet_plan_create()
    try:
        assert lib.glsdet_plan_begin(plan) == 0
        try:
            rc = call()
        finally:
            assert lib.glsdet_plan_end(plan) == 0
        if rc != 0:
            return "REFUSED: " + lib.glsdet_last_error().decode(errors="replace")
        assert lib.glsdet_plan_num_ops(plan) == 1
        name = C.create_string_buffer(256)
        assert lib.glsdet_plan_op_info(plan, 0, None, None, None, name, 256) == 0
        return name.value.decode()
    finally:
        lib.glsdet_plan_destroy(plan)


def rows():
    """[(entry point, case, hint, outcome)] from the library as built, in a fixed order"""
    from glsdet_amd import _lib
    lib = _lib.load()
    out = []
    for hint in HINTS:
        for name in PROBLEMS:
            d = _desc(_lib, _lib.ConvDesc(), name, hint)
            out.append(("conv2d", name, hint, _recorded(_lib, lib, lambda: lib.glsdet_conv2d(C.byref(d), None))))
        for name, (problem, c0, cin2, cout2, flags) in CHAINS.items():
            d = _desc(_lib, _lib.ConvDesc(), problem, hint)
            ch = _lib.ConvChain()
            ch.y2 = _view(_lib, d.y.n, d.y.h, d.y.w, cout2, d.y.dtype, 0x90000000)
            ch.w2, ch.scale2, ch.bias2 = 0xA0000000, 0xA0800000, 0xA0900000
            ch.act2, ch.c0, ch.cin2, ch.flags = 1, c0, cin2, flags
            out.append(("conv2d_chain", name, hint,
                        _recorded(_lib, lib, lambda: lib.glsdet_conv2d_chain(C.byref(d), C.byref(ch), None))))
        for name, (problem, extents) in MULTIS.items():
            ds = (_lib.ConvDesc * len(extents))()
            for i, hw in enumerate(extents):
                _desc(_lib, ds[i], problem, hint, slot=i, out_hw=hw)
            out.append(("conv2d_multi", name, hint,
                        _recorded(_lib, lib, lambda: lib.glsdet_conv2d_multi(ds, len(extents), None))))
        for name, (problem, groups) in GNSTATS.items():
            d = _desc(_lib, _lib.ConvDesc(), problem, hint)
            out.append(("conv2d_gnstats", name, hint,
                        _recorded(_lib, lib, lambda: lib.glsdet_conv2d_gnstats(C.byref(d), groups, 0xB0000000, None))))
    return out


def grouped(table):
    """{"entry case": {outcome: [hints]}}: the fixture's form (one line per outcome of a case)"""
    out = {}
    for entry, case, hint, op in table:
        # (a refusal's wording is not pinned, and texts that name the hint would not group: only the outcome is kept)
        out.setdefault(entry + " " + case, {}).setdefault("REFUSED" if op.startswith("REFUSED") else op, []).append(hint)
    return out


def main(out=OUT):
    g = grouped(rows())
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": {\n" + ",\n".join("  %s: %s" % (json.dumps(op), json.dumps(hs)) for op, hs in v.items()) + "\n}"
                                  for k, v in g.items()) + "\n}\n")
    print("wrote %s: %d cases, %d bytes" % (out, len(g), os.path.getsize(out)))


if __name__ == "__main__":
    main(*sys.argv[1:2])
