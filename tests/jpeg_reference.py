"""A slow and obvious numpy restatement of baseline JPEG decoding as libjpeg(-turbo) with JDCT_ISLOW and fancy upsampling
does it -- what `PIL.Image.open(...).convert("RGB")` gives: marker parser, bit-by-bit Huffman, jidctint.c's inverse DCT in
64-bit integers, jdsample.c's triangle filters and jdcolor.c's fixed-point colour conversion.  It handles the streams
the library accepts (SOF0, one interleaved scan, grayscale / 4:4:4 / 4:2:2 / 4:2:0) and asserts on anything else.

`mistakes` (a set of names from MISTAKES) plants one plausible error each, so that the tests can show which case sees it.

CASES is the list of encoder settings the CPU and the GPU tests share; `encode(case)` makes the bytes with Pillow."""
import io
import zlib

import numpy as np

MISTAKES = ("swap78", "triangle_narrow", "no_edge_rows", "no_half_g", "rows_first", "zigzag_t", "dc_no_reset",
            "keep_stuffing", "crop_after")

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
          41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


# ------------------------------------------------------------------------------------------------ markers
def parse(data: bytes) -> dict:
    """-> the fields of glsdet_jpeg_desc plus the tables: qt {id: uint16 [64] natural order}, dc / ac {id: {(length,
    code): symbol}}"""
    assert data[:2] == b"\xff\xd8"
    pos = 2
    info = {"restart_interval": 0, "qt": {}, "dc": {}, "ac": {}}
    while True:
        assert data[pos] == 0xFF
        while data[pos + 1] == 0xFF:
            pos += 1
        m = data[pos + 1]
        length = (data[pos + 2] << 8) | data[pos + 3]
        seg = data[pos + 4:pos + 2 + length]
        pos += 2 + length
        if m == 0xDB:
            while seg:
                assert seg[0] >> 4 == 0
                t = np.zeros(64, np.uint16)
                for k in range(64):
                    t[ZIGZAG[k]] = seg[1 + k]
                info["qt"][seg[0] & 15] = t
                seg = seg[65:]
        elif m == 0xC4:
            while seg:
                counts = list(seg[1:17])
                syms = seg[17:17 + sum(counts)]
                table, code, k = {}, 0, 0
                for ln in range(1, 17):
                    for _ in range(counts[ln - 1]):
                        table[(ln, code)] = syms[k]
                        code += 1
                        k += 1
                    code <<= 1
                info["ac" if seg[0] >> 4 else "dc"][seg[0] & 15] = table
                seg = seg[17 + sum(counts):]
        elif m == 0xDD:
            info["restart_interval"] = (seg[0] << 8) | seg[1]
        elif m == 0xC0:
            assert seg[0] == 8
            info["height"], info["width"], nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            assert nc in (1, 3)
            info["ncomp"] = nc
            info["hs"] = [seg[7 + 3 * c] >> 4 for c in range(nc)] + [0] * (3 - nc)
            info["vs"] = [seg[7 + 3 * c] & 15 for c in range(nc)] + [0] * (3 - nc)
            info["tq"] = [seg[8 + 3 * c] for c in range(nc)] + [0] * (3 - nc)
        elif m == 0xDA:
            nc = info["ncomp"]
            assert seg[0] == nc
            info["td"] = [seg[2 + 2 * c] >> 4 for c in range(nc)] + [0] * (3 - nc)
            info["ta"] = [seg[2 + 2 * c] & 15 for c in range(nc)] + [0] * (3 - nc)
            info["scan_offset"] = pos
            break
        else:
            assert m not in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF), "not baseline"
    hs, vs = info["hs"], info["vs"]
    info["mcus_x"] = -(-info["width"] // (8 * hs[0]))
    info["mcus_y"] = -(-info["height"] // (8 * vs[0]))
    info["blocks_x"] = [info["mcus_x"] * h for h in hs]
    info["blocks_y"] = [info["mcus_y"] * v for v in vs]
    info["n_blocks"] = sum(a * b for a, b in zip(info["blocks_x"], info["blocks_y"]))
    return info


# ------------------------------------------------------------------------------------------------ Huffman
class _Bits:
    def __init__(self, data, pos, keep_stuffing):
        self.data, self.pos, self.keep = data, pos, keep_stuffing
        self.byte, self.left = 0, 0

    def bit(self):
        if self.left == 0:
            self.byte = self.data[self.pos]
            self.pos += 1
            if self.byte == 0xFF:
                assert self.data[self.pos] == 0x00, "marker inside the entropy-coded data"
                if not self.keep:
                    self.pos += 1                  # the stuffed zero is no data
            self.left = 8
        self.left -= 1
        return (self.byte >> self.left) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for ln in range(1, 17):
            code = (code << 1) | self.bit()
            if (ln, code) in table:
                return table[(ln, code)]
        raise AssertionError("no such Huffman code")

    def value(self, s):
        v = self.bits(s)
        return v if v >= (1 << (s - 1)) else v - (1 << s) + 1

    def restart(self, expect):
        self.left = 0
        assert self.data[self.pos] == 0xFF and self.data[self.pos + 1] == 0xD0 + expect
        self.pos += 2


def entropy_decode(data: bytes, info: dict, mistakes=()):
    """-> (coef int16 [n_blocks, 64]: component by component, block raster, natural order, not dequantised;
    qtab uint16 [3, 64]: the table of each component, zero rows for absent ones)"""
    nc = info["ncomp"]
    coef = np.zeros((info["n_blocks"], 64), np.int16)
    qtab = np.zeros((3, 64), np.uint16)
    base = [0, 0, 0]
    for c in range(nc):
        qtab[c] = info["qt"][info["tq"][c]]
        if c:
            base[c] = base[c - 1] + info["blocks_x"][c - 1] * info["blocks_y"][c - 1]
    zz = ZIGZAG
    if "zigzag_t" in mistakes:
        zz = [(i % 8) * 8 + i // 8 for i in ZIGZAG]
    br = _Bits(data, info["scan_offset"], "keep_stuffing" in mistakes)
    pred = [0, 0, 0]
    ri, rst = info["restart_interval"], 0
    for mcu in range(info["mcus_x"] * info["mcus_y"]):
        if ri and mcu and mcu % ri == 0:
            br.restart(rst)
            rst = (rst + 1) % 8
            if "dc_no_reset" not in mistakes:
                pred = [0, 0, 0]
        my, mx = divmod(mcu, info["mcus_x"])
        for c in range(nc):
            dc, ac = info["dc"][info["td"][c]], info["ac"][info["ta"][c]]
            for v in range(info["vs"][c]):
                for h in range(info["hs"][c]):
                    out = coef[base[c] + (my * info["vs"][c] + v) * info["blocks_x"][c] + mx * info["hs"][c] + h]
                    s = br.symbol(dc)
                    pred[c] += br.value(s) if s else 0
                    out[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = br.symbol(ac)
                        run, size = rs >> 4, rs & 15
                        if size == 0:
                            if run != 15:
                                break
                            k += 16
                            continue
                        k += run
                        out[zz[k]] = br.value(size)
                        k += 1
    return coef, qtab


# ------------------------------------------------------------------------------------------------ inverse DCT
def _butterfly(i):
    """jidctint.c's 1-D pass on eight int64 arrays -> eight int64 arrays (not descaled)"""
    z1 = (i[2] + i[6]) * 4433
    tmp2 = z1 - i[6] * 15137
    tmp3 = z1 + i[2] * 6270
    tmp0 = (i[0] + i[4]) << 13
    tmp1 = (i[0] - i[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3 = z3 * -16069 + z5
    z4 = z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    return [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]


def idct_blocks(coef, q, mistakes=()):
    """coef int16 [n, 64], q uint16 [64] (both natural order) -> uint8 [n, 8, 8]: dequantise, pass 1 down the columns
    (descale 11), pass 2 along the rows (descale 18), + 128, saturate"""
    d = (coef.astype(np.int64) * q.astype(np.int64)[None, :]).reshape(-1, 8, 8)
    if "rows_first" in mistakes:
        d = d.transpose(0, 2, 1)
    ws = np.stack(_butterfly([d[:, k, :] for k in range(8)]), axis=1)          # [n, k, col]
    ws = (ws + (1 << 10)) >> 11
    out = np.stack(_butterfly([ws[:, :, k] for k in range(8)]), axis=2)        # [n, row, k]
    out = ((out + (1 << 17)) >> 18) + 128
    if "rows_first" in mistakes:
        out = out.transpose(0, 2, 1)
    return np.clip(out, 0, 255).astype(np.uint8)


def planes(info, coef, qtab, mistakes=()):
    """-> one uint8 plane per component, padded to whole MCUs"""
    out, b0 = [], 0
    for c in range(info["ncomp"]):
        bx, by = info["blocks_x"][c], info["blocks_y"][c]
        blk = idct_blocks(coef[b0:b0 + bx * by], qtab[c], mistakes)
        out.append(blk.reshape(by, bx, 8, 8).transpose(0, 2, 1, 3).reshape(by * 8, bx * 8))
        b0 += bx * by
    return out


# ------------------------------------------------------------------------------------------------ upsampling, colour
def upsample(plane, W, H, hs, vs, mistakes=()):
    """jdsample.c on the REAL samples of a chroma plane (dw x dh), cropped to W x H.  hs, vs: the luma factors."""
    if hs == 1:
        return plane[:H, :W].astype(np.int64)
    dw, dh = -(-W // hs), -(-H // vs)
    if "crop_after" in mistakes:
        dw, dh = plane.shape[1], plane.shape[0]
    p = plane[:dh, :dw].astype(np.int64)
    if dw <= 2 and "triangle_narrow" not in mistakes:
        return np.repeat(np.repeat(p, vs, axis=0), hs, axis=1)[:H, :W]
    if vs == 1:
        rows = [p]
    else:
        up = np.concatenate([p[:1], p[:-1]], 0)            # row r-1, the top edge replicated
        dn = np.concatenate([p[1:], p[-1:]], 0)            # row r+1, the bottom edge replicated
        if "no_edge_rows" in mistakes:
            up = np.concatenate([p[1:2] if dh > 1 else p[:1], p[:-1]], 0)
            dn = np.concatenate([p[1:], plane[dh:dh + 1, :dw].astype(np.int64) if plane.shape[0] > dh else p[-2:-1]], 0)
        rows = [3 * p + up, 3 * p + dn]
    outs = []
    for v, s in enumerate(rows):
        left = np.concatenate([s[:, :1], s[:, :-1]], 1)    # s[c-1], an edge column is its own neighbour
        right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
        if vs == 1:
            even, odd = (3 * s + left + 1) >> 2, (3 * s + right + 2) >> 2
        else:
            a, b = (7, 8) if "swap78" in mistakes else (8, 7)
            even, odd = (3 * s + left + a) >> 4, (3 * s + right + b) >> 4
        o = np.empty((dh, 2 * dw), np.int64)
        o[:, 0::2], o[:, 1::2] = even, odd
        outs.append(o)
    if vs == 1:
        return outs[0][:H, :W]
    full = np.empty((2 * dh, 2 * dw), np.int64)
    full[0::2], full[1::2] = outs
    return full[:H, :W]


def reconstruct(info, coef, qtab, order="rgb", mistakes=()):
    """-> uint8 [H, W, 3]"""
    W, H = info["width"], info["height"]
    pl = planes(info, coef, qtab, mistakes)
    Y = pl[0][:H, :W].astype(np.int64)
    if info["ncomp"] == 1:
        return np.stack([Y, Y, Y], 2).astype(np.uint8)
    cb = upsample(pl[1], W, H, info["hs"][0], info["vs"][0], mistakes) - 128
    cr = upsample(pl[2], W, H, info["hs"][0], info["vs"][0], mistakes) - 128
    half = 0 if "no_half_g" in mistakes else 32768
    R = Y + ((91881 * cr + 32768) >> 16)
    G = Y + ((-22554 * cb - 46802 * cr + half) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    rgb = np.clip(np.stack([R, G, B], 2), 0, 255).astype(np.uint8)
    return rgb[:, :, ::-1].copy() if order == "bgr" else rgb


def decode(data: bytes, order="rgb", mistakes=()):
    info = parse(data)
    coef, qtab = entropy_decode(data, info, mistakes)
    return reconstruct(info, coef, qtab, order, mistakes)


# ------------------------------------------------------------------------------------------------ the shared cases
SIZES = [(1, 1), (8, 8), (9, 2), (16, 1), (2, 4), (3, 3), (33, 3), (15, 31), (17, 33), (37, 53), (64, 80)]   # (W, H)
QUALITIES = (30, 95, 100)


def picture(w, h, kind, seed, gray=False):
    """'smooth': gradients plus a little texture; 'noise': uniform noise (every coefficient alive)"""
    rng = np.random.RandomState(seed)
    ch = 1 if gray else 3
    if kind == "noise":
        a = rng.randint(0, 256, (h, w, ch))
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([(xx * (5 + 3 * c) + yy * (11 - 2 * c) + 40 * c) % 256 for c in range(ch)], 2) + rng.randint(-6, 7, (h, w, ch))
    a = np.clip(a, 0, 255).astype(np.uint8)
    return a[:, :, 0] if gray else a


def _cases():
    out = []

    def add(name, w, h, kind, **kw):
        out.append({"name": "%s-%dx%d-%s" % (name, w, h, kind), "w": w, "h": h, "kind": kind, "save": kw})
    for i, (w, h) in enumerate(SIZES):
        for ss in (0, 1, 2):
            add("ss%d-q%d" % (ss, QUALITIES[(i + ss) % 3]), w, h, ("smooth", "noise")[(i + ss) % 2], subsampling=ss,
                quality=QUALITIES[(i + ss) % 3])
    for (w, h) in ((9, 2), (17, 33), (3, 3), (2, 4)):
        for ss in (0, 1, 2):
            for q in QUALITIES:
                add("ss%d-q%d-x" % (ss, q), w, h, "noise" if q != 95 else "smooth", subsampling=ss, quality=q)
    for i, (w, h) in enumerate(SIZES):
        add("gray-q%d" % QUALITIES[i % 3], w, h, ("noise", "smooth")[i % 2], quality=QUALITIES[i % 3], gray=True)
    for i, (w, h) in enumerate(((17, 33), (37, 53), (33, 3), (64, 80))):
        for j, rs in enumerate(({"restart_marker_blocks": 1}, {"restart_marker_blocks": 2}, {"restart_marker_rows": 1})):
            add("rst-%s%d-ss%d" % (list(rs)[0][15:], list(rs.values())[0], (i + j) % 3), w, h, ("noise", "smooth")[j % 2],
                subsampling=(i + j) % 3, quality=(95, 30, 100)[j], **rs)
    add("rst-blocks2-gray", 37, 53, "noise", quality=95, gray=True, restart_marker_blocks=2)
    for ss in (0, 1, 2):
        add("optimize-ss%d" % ss, 37, 53, "noise", subsampling=ss, quality=95, optimize=True)
    add("optimize-gray", 15, 31, "smooth", quality=30, gray=True, optimize=True)
    for ss in (0, 1, 2):
        add("q1-ss%d" % ss, 17, 33, "noise", subsampling=ss, qtables=[[1] * 64, [1] * 64])
        add("q255-ss%d" % ss, 17, 33, "noise", subsampling=ss, qtables=[[255] * 64, [255] * 64])
    add("app1-com-ss2", 37, 53, "smooth", subsampling=2, quality=95, exif=b"Exif\x00\x00" + bytes(range(256)) * 200,
        comment=b"a comment segment " * 40)
    return out


CASES = _cases()
_encoded = {}


def encode(case) -> bytes:
    """the case's bytes from Pillow's encoder (cached)"""
    from PIL import Image
    if case["name"] not in _encoded:
        kw = dict(case["save"])
        gray = kw.pop("gray", False)
        img = Image.fromarray(picture(case["w"], case["h"], case["kind"], zlib.crc32(case["name"].encode()), gray))
        b = io.BytesIO()
        img.save(b, "JPEG", **kw)
        _encoded[case["name"]] = b.getvalue()
    return _encoded[case["name"]]


def pillow(data: bytes, order="rgb"):
    from PIL import Image
    a = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    return a[:, :, ::-1].copy() if order == "bgr" else a
