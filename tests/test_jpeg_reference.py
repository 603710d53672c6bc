"""CPU: the baseline JPEG decoder's host half and the restatement the GPU tests rest on.

* tests/jpeg_reference.py (numpy) == Pillow, exactly, on the shared case list; each planted mistake is seen by a named case;
* glsdet_jpeg_parse / glsdet_jpeg_entropy_decode (host only, no GPU) == the restatement, bit for bit, into sentinel-filled
  buffers compared whole;
* every refusal the header lists, made by patching bytes of a Pillow stream, returns a negative code whose message names
  the cause; every proper prefix of a small 4:2:0 stream with restart markers is refused; every single-byte substitution
  of it returns success or a negative code with the guard bytes around the buffers intact;
* JpegDecoder.probe and the fallback switch as far as they go without a device."""
import ctypes as C
import io

import numpy as np
import pytest

from tests import jpeg_reference as R

GUARD = 64
SENT16 = 0x5A5A


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from glsdet_amd import _lib
    return _lib.load()


def _ids(cases):
    return [c["name"] for c in cases]


# ------------------------------------------------------------------------------------------------ restatement == Pillow
@pytest.mark.parametrize("case", R.CASES, ids=_ids(R.CASES))
def test_restatement_equals_pillow(case):
    data = R.encode(case)
    want = R.pillow(data)
    assert want.shape == (case["h"], case["w"], 3)
    got = R.decode(data)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(R.decode(data, order="bgr"), want[:, :, ::-1])


def test_case_list_covers_what_it_should():
    names = _ids(R.CASES)
    assert len(names) == len(set(names)) and 95 <= len(names) <= 130
    for (w, h) in R.SIZES:
        for ss in (0, 1, 2):
            assert any(c["w"] == w and c["h"] == h and c["save"].get("subsampling") == ss for c in R.CASES)
        assert any(c["w"] == w and c["h"] == h and c["save"].get("gray") for c in R.CASES)
    for key in ("restart_marker_blocks", "restart_marker_rows", "optimize", "qtables", "exif", "comment"):
        assert any(key in c["save"] for c in R.CASES), key
    big = R.encode(next(c for c in R.CASES if "exif" in c["save"]))
    assert b"\xff\xe1" in big and b"\xff\xfe" in big and len(big) > 50000


# the case that sees each planted mistake (found by running every mistake over the list; several see most of them)
MISTAKE_CASE = {
    "swap78": "ss2-q95-17x33-smooth",
    "triangle_narrow": "ss2-q95-3x3-noise",
    "no_edge_rows": "ss2-q100-33x3-smooth",
    "no_half_g": "ss0-q95-8x8-noise",
    "rows_first": "ss0-q95-8x8-noise",
    "zigzag_t": "ss1-q100-8x8-smooth",
    "dc_no_reset": "rst-blocks1-ss0-17x33-noise",
    "keep_stuffing": "ss1-q100-8x8-smooth",
    "crop_after": "ss2-q30-8x8-noise",
}


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_each_planted_mistake_is_seen_by_its_case(mistake):
    case = next(c for c in R.CASES if c["name"] == MISTAKE_CASE[mistake])
    data = R.encode(case)
    want = R.pillow(data)
    assert np.array_equal(R.decode(data), want)
    try:
        got = R.decode(data, mistakes={mistake})
    except (AssertionError, IndexError, KeyError):
        return                                             # a mistake in the bit stream may lose the stream altogether
    assert not np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ library == restatement
FIELDS = ("width", "height", "ncomp", "hs", "vs", "mcus_x", "mcus_y", "restart_interval", "blocks_x", "blocks_y", "n_blocks",
          "scan_offset", "tq", "td", "ta")


def _field(d, k):
    v = getattr(d, k)
    return v if isinstance(v, int) else list(v)


def _parse(lib, data):
    from glsdet_amd._lib import JpegDesc
    d = JpegDesc()
    buf = (C.c_ubyte * max(len(data), 1)).from_buffer_copy(data or b"\0")     # exactly nbytes long: no terminator to lean on
    return lib.glsdet_jpeg_parse(buf, len(data), C.byref(d)), d, buf


def _entropy(lib, buf, nbytes, d, n_blocks=None):
    """-> (rc, coef with its guards, qtab with its guards)"""
    n = (d.n_blocks if n_blocks is None else n_blocks) * 64
    coef = np.full(n + 2 * GUARD, SENT16, np.int16)
    qtab = np.full(192 + 2 * GUARD, SENT16, np.uint16)
    rc = lib.glsdet_jpeg_entropy_decode(buf, nbytes, C.byref(d), coef[GUARD:].ctypes.data, qtab[GUARD:].ctypes.data)
    return rc, coef, qtab


def _guards_intact(coef, qtab):
    return bool((coef[:GUARD] == SENT16).all() and (coef[-GUARD:] == SENT16).all() and (qtab[:GUARD] == SENT16).all() and
                (qtab[-GUARD:] == SENT16).all())


@pytest.mark.parametrize("case", R.CASES, ids=_ids(R.CASES))
def test_library_parse_and_entropy_equal_the_restatement(lib, case):
    data = R.encode(case)
    info = R.parse(data)
    rc, d, buf = _parse(lib, data)
    assert rc == 0, lib.glsdet_last_error()
    assert {k: _field(d, k) for k in FIELDS} == {k: info[k] for k in FIELDS}
    assert d.reserved == 0
    rc, coef, qtab = _entropy(lib, buf, len(data), d)
    assert rc == 0, lib.glsdet_last_error()
    want_c, want_q = R.entropy_decode(data, info)
    g16 = np.full(GUARD, SENT16, np.int16)
    assert np.array_equal(coef, np.concatenate([g16, want_c.reshape(-1), g16]))
    assert np.array_equal(qtab, np.concatenate([g16.astype(np.uint16), want_q.reshape(-1), g16.astype(np.uint16)]))


# ------------------------------------------------------------------------------------------------ refusals
def _save(arr, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, "JPEG", **kw)
    return b.getvalue()


def _segments(data):
    """[(marker, offset of its FF, length field)] up to and including SOS"""
    out, pos = [], 2
    while True:
        m, ln = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        out.append((m, pos, ln))
        if m == 0xDA:
            return out
        pos += 2 + ln


def _seg(data, marker):
    return next(s for s in _segments(data) if s[0] == marker)


def _patch(data, off, new):
    return data[:off] + bytes(new) + data[off + len(bytes(new)):]


def _without(data, marker):
    _, off, ln = _seg(data, marker)
    return data[:off] + data[off + 2 + ln:]


def _insert_before(data, marker, blob):
    _, off, _ = _seg(data, marker)
    return data[:off] + blob + data[off:]


def _craft(base, bits):
    """the stream `base` with its entropy-coded data replaced by the bit string `bits`, padded with ones and stuffed"""
    bits += "1" * (-len(bits) % 8)
    payload = b"".join(bytes([int(bits[i:i + 8], 2)]) + (b"\x00" if bits[i:i + 8] == "11111111" else b"") for i in range(0, len(bits), 8))
    return base[:R.parse(base)["scan_offset"]] + payload + b"\xff\xd9"


def _code(table, sym):
    ln, code = next(k for k, v in table.items() if v == sym)
    return format(code, "0%db" % ln)


def _refusal_streams():
    rgb = R.picture(17, 33, "noise", 7)
    base = _save(rgb, subsampling=2, quality=90)
    rst = _save(rgb, subsampling=2, quality=90, restart_marker_blocks=1)
    sof, sos, dqt = _seg(base, 0xC0)[1], _seg(base, 0xDA)[1], _seg(base, 0xDB)[1]
    out = {}
    out["SOF2 patched in"] = (_patch(base, sof + 1, [0xC2]), "progressive")
    out["Pillow progressive=True"] = (_save(rgb, progressive=True), "progressive")
    out["SOF1"] = (_patch(base, sof + 1, [0xC1]), "extended sequential")
    out["SOF9 arithmetic"] = (_patch(base, sof + 1, [0xC9]), "arithmetic")
    out["12-bit"] = (_patch(base, sof + 4, [12]), "12-bit")
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rgb).convert("CMYK").save(b, "JPEG")
    out["4 components (CMYK)"] = (b.getvalue(), "4 components")
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
    out["Adobe transform 0"] = (_insert_before(_without(base, 0xE0), 0xDB, adobe), "Adobe")
    ids = _patch(_patch(_patch(base, sof + 10, b"R"), sof + 13, b"G"), sof + 16, b"B")
    ids = _patch(_patch(_patch(ids, sos + 5, b"R"), sos + 7, b"G"), sos + 9, b"B")
    out["component ids R G B"] = (_without(ids, 0xE0), "RGB")
    out["4:4:0 sampling"] = (_patch(base, sof + 11, [0x12]), "sampling factors")
    out["4:1:1 sampling"] = (_patch(base, sof + 11, [0x41]), "sampling factors")
    out["chroma 2x1"] = (_patch(base, sof + 14, [0x21]), "sampling factors")
    out["scan of one component"] = (_patch(base, sos + 4, [1]), "several scans")
    out["second scan after the first"] = (base[:-2] + base[sos:], "several scans")
    out["16-bit DQT"] = (_patch(base, dqt + 4, [base[dqt + 4] | 0x10]), "16-bit")
    out["height 0"] = (_patch(base, sof + 5, [0, 0]), "height 0")
    out["DNL"] = (_insert_before(base, 0xDA, b"\xff\xdc\x00\x04\x00\x21"), "DNL")
    out["DC selector without table"] = (_patch(base, sos + 6, [0x30 | (base[sos + 6] & 15)]), "no DHT defines")
    out["AC selector without table"] = (_patch(base, sos + 6, [(base[sos + 6] & 0xF0) | 3]), "no DHT defines")
    out["Tq without table"] = (_patch(base, sof + 12, [3]), "no DQT defines")
    out["more than 2^28 pixels"] = (_patch(base, sof + 5, [0x40, 0x00, 0x80, 0x00]), "2^28")
    out["no SOI"] = (b"\x89PNG\r\n\x1a\n" + base, "not a JPEG")
    # entropy-stage refusals
    scan = R.parse(rst)["scan_offset"]
    first = rst.index(b"\xff\xd0", scan)
    out["RST out of order"] = (_patch(rst, first + 1, [0xD1]), "out-of-order")
    out["RST missing"] = (_patch(rst, first, [0x12, 0x34]), "missing RST0")
    out["cut inside the scan"] = (base[:scan + (len(base) - scan) // 2], "ends before the last MCU")
    out["cut before EOI"] = (base[:-2], "before the EOI")
    gray = _save(R.picture(16, 8, "smooth", 3, gray=True), quality=90)          # two blocks, the standard tables
    gi = R.parse(gray)
    dc, ac = gi["dc"][0], gi["ac"][0]
    eob, zrl = _code(ac, 0x00), _code(ac, 0xF0)
    out["code in no table"] = (_craft(gray, "1" * 64), "in no table")
    out["run past 63 (ZRL)"] = (_craft(gray, _code(dc, 0) + zrl * 4 + eob + _code(dc, 0) + eob), "past coefficient 63")
    out["run past 63 (run + size)"] = (_craft(gray, _code(dc, 0) + zrl * 3 + _code(ac, 0xF1) + "1" + eob + _code(dc, 0) + eob),
                                       "past coefficient 63")
    big = _code(dc, 11) + "1" * 11 + eob                                         # DC difference +2047
    out["DC outside [-2048, 2047]"] = (_craft(gray, big + big), "outside [-2048, 2047]")
    # an AC table whose only codes are EOB and run 0 / size 12: the first value read is +4095
    ac_off = next(off for m, off, ln in _segments(gray) if m == 0xC4 and gray[off + 4] >> 4 == 1)
    small = b"\xff\xc4\x00\x15\x10" + bytes([2] + [0] * 15) + b"\x00\x0c"
    own = gray[:ac_off] + small + gray[ac_off + 2 + ((gray[ac_off + 2] << 8) | gray[ac_off + 3]):]
    assert R.parse(own)["ac"][0] == {(1, 0): 0x00, (1, 1): 0x0C}
    out["AC outside [-2048, 2047]"] = (_craft(own, _code(dc, 0) + "1" + "1" * 12 + "0" + _code(dc, 0) + "0"), "outside [-2048, 2047]")
    return out


_REFUSALS = _refusal_streams()


@pytest.mark.parametrize("name", list(_REFUSALS))
def test_refusals_name_their_cause(lib, name):
    data, cause = _REFUSALS[name]
    rc, d, buf = _parse(lib, data)
    if rc == 0:
        rc, coef, qtab = _entropy(lib, buf, len(data), d)
        assert _guards_intact(coef, qtab)
    msg = lib.glsdet_last_error().decode()
    assert rc < 0 and cause in msg, (rc, msg)


def test_refused_streams_are_the_ones_pillow_or_the_contract_rules_out(lib):
    """the patched streams are not accidentally broken elsewhere: the unpatched bases decode, and equal Pillow"""
    rgb = R.picture(17, 33, "noise", 7)
    for kw in ({}, {"restart_marker_blocks": 1}):
        data = _save(rgb, subsampling=2, quality=90, **kw)
        rc, d, buf = _parse(lib, data)
        assert rc == 0
        rc, coef, qtab = _entropy(lib, buf, len(data), d)
        assert rc == 0 and np.array_equal(R.reconstruct(R.parse(data), coef[GUARD:-GUARD].reshape(-1, 64),
                                                        qtab[GUARD:-GUARD].reshape(3, 64)), R.pillow(data))


def test_null_and_mismatched_arguments(lib):
    from glsdet_amd._lib import JpegDesc
    data = _save(R.picture(9, 9, "noise", 1), quality=80)
    rc, d, buf = _parse(lib, data)
    assert rc == 0
    assert lib.glsdet_jpeg_parse(None, 10, C.byref(d)) < 0 and lib.glsdet_jpeg_parse(buf, len(data), None) < 0
    assert lib.glsdet_jpeg_parse(buf, -1, C.byref(JpegDesc())) < 0 and lib.glsdet_jpeg_parse(buf, 0, C.byref(JpegDesc())) < 0
    other = JpegDesc.from_buffer_copy(d)
    other.n_blocks += 1                                    # a descriptor that is not this stream's sizes nothing
    rc, coef, qtab = _entropy(lib, buf, len(data), other, n_blocks=d.n_blocks)
    assert rc < 0 and "descriptor" in lib.glsdet_last_error().decode()
    assert (coef == SENT16).all() and (qtab == SENT16).all()
    assert lib.glsdet_jpeg_entropy_decode(buf, len(data), C.byref(d), None, None) < 0


# ------------------------------------------------------------------------------------------------ sweeps
@pytest.fixture(scope="module")
def sweep_stream():
    data = _save(R.picture(17, 17, "noise", 11), subsampling=2, quality=25, restart_marker_blocks=1)
    assert 300 < len(data) < 1200 and data.count(b"\xff\xd0") >= 1
    return data


def _decode_rc(lib, data):
    rc, d, buf = _parse(lib, data)
    if rc:
        return rc, True
    rc, coef, qtab = _entropy(lib, buf, len(data), d)
    return rc, _guards_intact(coef, qtab)


def test_every_proper_prefix_is_refused(lib, sweep_stream):
    assert _decode_rc(lib, sweep_stream) == (0, True)
    for n in range(len(sweep_stream)):
        rc, intact = _decode_rc(lib, sweep_stream[:n])
        assert rc < 0 and intact, n


def test_every_single_byte_substitution_is_decoded_or_refused_inside_the_buffers(lib, sweep_stream):
    seen = set()
    for i in range(len(sweep_stream)):
        for v in (0x00, 0xFF, sweep_stream[i] ^ 0xFF):
            if v == sweep_stream[i]:
                continue
            rc, intact = _decode_rc(lib, _patch(sweep_stream, i, [v]))
            assert rc <= 0 and intact, (i, v)
            seen.add(rc < 0)
    assert seen == {True, False}                           # some substitutions are harmless (APP0 bytes), most are caught


# ------------------------------------------------------------------------------------------------ the Python surface
def test_probe_is_host_only(lib, tmp_path):
    from glsdet_amd.jpeg import JpegDecoder
    dec = JpegDecoder()
    for ss, name in ((0, "4:4:4"), (1, "4:2:2"), (2, "4:2:0")):
        data = _save(R.picture(37, 53, "smooth", 2), subsampling=ss, quality=80)
        p = dec.probe(data)
        assert (p["width"], p["height"], p["size"], p["mode"], p["subsampling"]) == (37, 53, (37, 53), "RGB", name)
    gray = _save(R.picture(9, 2, "smooth", 2, gray=True), restart_marker_blocks=2)
    path = tmp_path / "g.jpg"
    path.write_bytes(gray)
    want = {"width": 9, "height": 2, "size": (9, 2), "mode": "L", "subsampling": None, "restart_interval": 2}
    assert dec.probe(gray) == want and dec.probe(str(path)) == want and dec.probe(path) == want
    with open(path, "rb") as f:
        assert dec.probe(f) == want
    with pytest.raises(ValueError, match="progressive"):
        dec.probe(_save(R.picture(9, 9, "smooth", 2), progressive=True))
    with pytest.raises(TypeError):
        dec.probe(12)


def test_fallback_switch_without_a_device(lib):
    from glsdet_amd.jpeg import JpegDecoder, JpegRefused
    with pytest.raises(ValueError, match="fallback"):
        JpegDecoder(fallback="eager")
    prog = _save(R.picture(9, 9, "smooth", 2), progressive=True)
    dec = JpegDecoder(fallback="raise")
    with pytest.raises(ValueError, match="progressive") as e:          # the library's message, before any device is needed
        dec.decode(prog)
    assert isinstance(e.value, JpegRefused)
    with pytest.raises(ValueError, match="not a JPEG"):
        dec.decode(b"GIF89a" + bytes(40))
    with pytest.raises(ValueError, match="order"):
        dec.decode(prog, order="gbr")


def test_geometry_round_trip(lib):
    from glsdet_amd import jpeg as J
    for case in R.CASES[:12] + R.CASES[-20:]:
        d = J.parse(R.encode(case))
        g = J.desc_from_geometry(J.geometry(d))
        for k in ("width", "height", "ncomp", "hs", "vs", "mcus_x", "mcus_y", "blocks_x", "blocks_y", "n_blocks"):
            assert _field(g, k) == _field(d, k), (case["name"], k)
        assert lib.glsdet_jpeg_workspace_bytes(C.byref(g)) == (d.n_blocks * 64 + 15) // 16 * 16
    bad = J.desc_from_geometry([16, 16, 3, 1, 1, 1, 2, 1, 1])         # 4:4:0
    assert lib.glsdet_jpeg_workspace_bytes(C.byref(bad)) == 0
