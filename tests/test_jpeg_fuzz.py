"""GPU: glsdet_jpeg_reconstruct (dequantise + ISLOW inverse DCT, fancy upsampling + YCbCr -> RGB) and the JpegDecoder over
it, bit for bit against Pillow on the case list of tests/jpeg_reference.py (which tests/test_jpeg_reference.py holds to
Pillow and the library's host half to on the CPU), and against the numpy restatement for hand-made coefficients Pillow
cannot be asked about.  Every destination is a sentinel-filled buffer larger than the call needs and is compared whole."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from tests import jpeg_reference as R

pytestmark = pytest.mark.gpu
SENT = 0xA5
GUARD = 512


@pytest.fixture(scope="module")
def lib():
    from glsdet_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_decoded = {}


def _host(case):
    """(descriptor, coef, qtab, Pillow's RGB) of a case: the library's host half and the reference, once"""
    from glsdet_amd import jpeg as J
    if case["name"] not in _decoded:
        data = R.encode(case)
        d = J.parse(data)
        coef, qtab = J.entropy_decode(data, d)
        _decoded[case["name"]] = (d, coef, qtab, R.pillow(data))
    return _decoded[case["name"]]


def _reconstruct(lib, desc, coef_h, qtab_h, order=0, pad=5, dirty=0xFF, **bad):
    """one call into a sentinel-filled destination with dst_row_bytes = 3*W + pad -> (rc, the whole destination [H + guard
    rows, 3*W + pad]); `bad` overrides single arguments for the refusal tests"""
    nws = lib.glsdet_jpeg_workspace_bytes(C.byref(desc))
    ws = torch.full((max(nws, 16) + 16,), dirty, dtype=torch.uint8, device="cuda")
    row = 3 * desc.width + pad
    dst = torch.full((desc.height * row + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    cd, qd = _dev(coef_h.reshape(-1)), _dev(qtab_h.reshape(-1).view(np.int16))
    a = {"d": C.byref(desc), "coef": cd.data_ptr(), "qtab": qd.data_ptr(), "ws": ws.data_ptr(), "ws_bytes": nws, "dst": dst.data_ptr(),
         "row": row, "order": order}
    a.update(bad)
    rc = lib.glsdet_jpeg_reconstruct(a["d"], a["coef"], a["qtab"], a["ws"], a["ws_bytes"], a["dst"], a["row"], a["order"], _stream())
    torch.cuda.synchronize()
    return rc, dst.cpu().numpy()


def _expected(rgb, pad=5):
    h, w = rgb.shape[:2]
    row = 3 * w + pad
    want = np.full(h * row + GUARD, SENT, np.uint8)
    want[:h * row].reshape(h, row)[:, :3 * w] = rgb.reshape(h, 3 * w)
    return want


# ------------------------------------------------------------------------------------------------ against Pillow
@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_reconstruct_equals_pillow_in_both_orders(lib, case):
    d, coef, qtab, rgb = _host(case)
    for order, want in ((0, rgb), (1, rgb[:, :, ::-1])):
        rc, got = _reconstruct(lib, d, coef, qtab, order, dirty=0xFF if order else 0x00)
        assert rc == 0, lib.glsdet_last_error()
        assert np.array_equal(got, _expected(want))


@pytest.mark.parametrize("pad", [0, 1, 2, 3])
def test_every_row_alignment_takes_its_store_path(lib, pad):
    """dst_row_bytes = 3*W + pad with W odd and even: rows start at every offset modulo 4 (dword and byte stores)"""
    for name in ("ss2-q100-37x53-noise", "ss1-q100-64x80-noise", "gray-q95-15x31-smooth"):
        d, coef, qtab, rgb = _host(next(c for c in R.CASES if c["name"] == name))
        rc, got = _reconstruct(lib, d, coef, qtab, 0, pad=pad)
        assert rc == 0 and np.array_equal(got, _expected(rgb, pad))


@pytest.mark.parametrize("ss,size", [(2, (512, 384)), (1, (512, 384)), (2, (2400, 2400))],
                         ids=["420-384x512", "422-384x512", "420-2400x2400-past-both-grid-caps"])
def test_larger_pictures_against_pillow_directly(lib, ss, size):
    """the last one holds 135 000 blocks and 5.76 M pixels: more than the 4096 thread blocks of either kernel cover in one
    sweep (32 blocks / 1024 pixels per thread block), so both grid-stride loops go round"""
    from glsdet_amd import jpeg as J
    from PIL import Image
    w, h = size
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.RandomState(w + ss)
    img = np.stack([(xx * 3 + yy) % 256, (xx + yy * 2) % 256, (xx * yy // 64) % 256], 2) + rng.randint(-20, 21, (h, w, 3))
    b = io.BytesIO()
    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(b, "JPEG", subsampling=ss, quality=90)
    data = b.getvalue()
    d = J.parse(data)
    assert d.n_blocks > (4096 * 32 if w > 2000 else 0)
    coef, qtab = J.entropy_decode(data, d)
    rc, got = _reconstruct(lib, d, coef, qtab, 0)
    assert rc == 0 and np.array_equal(got, _expected(R.pillow(data)))


# ------------------------------------------------------------------------------------------------ hand-made coefficients
def _info(w, h, ncomp=1, hs=1, vs=1):
    from glsdet_amd import jpeg as J
    d = J.desc_from_geometry([w, h, ncomp, hs, 1 if ncomp == 3 else 0, 1 if ncomp == 3 else 0, vs, 1 if ncomp == 3 else 0,
                              1 if ncomp == 3 else 0])
    info = {k: (getattr(d, k) if isinstance(getattr(d, k), int) else list(getattr(d, k)))
            for k in ("width", "height", "ncomp", "hs", "vs", "mcus_x", "mcus_y", "blocks_x", "blocks_y", "n_blocks")}
    return d, info


def _hand_blocks():
    blocks = []
    for s in (1, -1):
        b = np.zeros(64, np.int64)
        b[0] = 2047 * s if s > 0 else -2048                   # a lone DC at either end of the range
        blocks.append(b)
        b = np.zeros(64, np.int64)
        b[63] = 2047 * s                                      # a lone coef[63]
        blocks.append(b)
        b = np.zeros(64, np.int64)
        b[63] = s
        blocks.append(b)
        i = np.arange(64)
        blocks.append(s * 2047 * (1 - 2 * ((i // 8 + i % 8) % 2)))           # checkerboard of +-2047: far past 0..255
        blocks.append(s * 2047 * (1 - 2 * (i % 2)))                          # alternating along the rows
        blocks.append(s * 2047 * (1 - 2 * ((i // 8) % 2)))                   # alternating down the columns
        blocks.append(np.full(64, -2048 if s < 0 else 2047))
    rng = np.random.RandomState(5)
    for _ in range(34):
        blocks.append(rng.randint(-2048, 2048, 64))
    return np.stack(blocks).astype(np.int16)


@pytest.mark.parametrize("q", [255, 1, 16])
def test_hand_made_blocks_equal_the_restatement_with_saturation(lib, q):
    """coefficients no encoder writes: |coef * q| up to 2^19, sums far outside 32 bits in the passes and outside 0..255
    after them.  The result is the 64-bit restatement's, saturated (libjpeg's scalar code masks a table index there and
    its SIMD code saturates: that regime is defined here as saturation)"""
    coef = _hand_blocks()
    n = len(coef)
    d, info = _info(8 * n, 8)
    assert info["n_blocks"] == n
    qtab = np.zeros((3, 64), np.uint16)
    qtab[0] = q
    want = R.reconstruct(info, coef, qtab)
    assert want.min() == 0 and want.max() == 255
    rc, got = _reconstruct(lib, d, coef, qtab)
    assert rc == 0 and np.array_equal(got, _expected(want))
    # the same blocks as the three components of a 4:2:0 picture (chroma at the extremes of the colour conversion)
    d3, info3 = _info(16 * 3, 16 * 2, 3, 2, 2)
    nb = info3["n_blocks"]
    coef3 = np.concatenate([coef] * (nb // n + 1))[:nb]
    q3 = np.full((3, 64), q, np.uint16)
    rc, got = _reconstruct(lib, d3, coef3, q3, 1)
    assert rc == 0 and np.array_equal(got, _expected(R.reconstruct(info3, coef3, q3, "bgr")))


# ------------------------------------------------------------------------------------------------ host refusals
def test_every_host_refusal_launches_nothing(lib):
    from glsdet_amd._lib import JpegDesc
    case = next(c for c in R.CASES if c["name"] == "ss2-q95-17x33-smooth")
    d, coef, qtab, rgb = _host(case)
    untouched = np.full(d.height * (3 * d.width + 5) + GUARD, SENT, np.uint8)

    def refused(cause, desc=None, **bad):
        if desc is not None:
            bad["d"] = C.byref(desc)
        rc, got = _reconstruct(lib, d, coef, qtab, **bad)
        msg = lib.glsdet_last_error().decode()
        assert rc < 0 and cause in msg and np.array_equal(got, untouched), (bad, rc, msg)

    for k in ("coef", "qtab", "ws", "dst"):
        refused("null", **{k: None})
    refused("null", d=None)
    nws = lib.glsdet_jpeg_workspace_bytes(C.byref(d))
    assert nws == d.n_blocks * 64
    refused("workspace", ws_bytes=nws - 64)
    refused("workspace", ws_bytes=0)
    ws = torch.zeros(nws + 32, dtype=torch.uint8, device="cuda")
    refused("aligned", ws=ws.data_ptr() + 8)
    refused("dst_row_bytes", row=3 * d.width - 1)
    refused("dst_row_bytes", row=0)
    for order in (2, -1, 256):
        refused("order", order=order)

    def edit(**kw):
        e = JpegDesc.from_buffer_copy(d)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(e, k)[v[0]] = v[1]
            else:
                setattr(e, k, v)
        return e

    for e in (edit(n_blocks=d.n_blocks + 1), edit(n_blocks=d.n_blocks - 1), edit(mcus_x=d.mcus_x + 1), edit(mcus_y=d.mcus_y - 1),
              edit(blocks_x=(0, d.blocks_x[0] + 2)), edit(blocks_y=(2, d.blocks_y[2] + 1)), edit(blocks_x=(1, 0)),
              edit(width=d.width + 16), edit(height=d.height + 16)):
        refused("inconsistent descriptor", desc=e)
    for e, cause in ((edit(hs=(0, 3)), "sampling factors"), (edit(vs=(1, 2)), "sampling factors"), (edit(ncomp=2), "2 components"),
                     (edit(ncomp=4), "4 components"), (edit(width=0), "bad picture size"), (edit(height=-5), "bad picture size"),
                     (edit(width=65535, height=65535), "2^28"), (edit(width=1 << 20), "bad picture size")):
        refused(cause, desc=e)
    rc, got = _reconstruct(lib, d, coef, qtab)                     # and the untouched call still works
    assert rc == 0 and np.array_equal(got, _expected(rgb))


# ------------------------------------------------------------------------------------------------ plan, graph, torch op
def test_recorded_in_a_plan_and_replayed_from_a_captured_graph_on_new_coefficients(lib):
    from glsdet_amd import jpeg as J
    from glsdet_amd.engine import Plan
    from PIL import Image
    streams = []
    for seed in (1, 2):
        b = io.BytesIO()
        Image.fromarray(R.picture(37, 53, "noise", seed)).save(b, "JPEG", subsampling=2, quality=85)
        streams.append(b.getvalue())
    da, ca, qa = (J.parse(streams[0]),) + J.entropy_decode(streams[0])
    db, cb, qb = (J.parse(streams[1]),) + J.entropy_decode(streams[1])
    assert J.geometry(da) == J.geometry(db) and not np.array_equal(ca, cb)
    want_a, want_b = R.pillow(streams[0]), R.pillow(streams[1])
    coef, qtab = _dev(ca.reshape(-1)), _dev(qa.reshape(-1).view(np.int16))
    ws = torch.empty(lib.glsdet_jpeg_workspace_bytes(C.byref(da)), dtype=torch.uint8, device="cuda")
    dst = torch.full((53, 37, 3), SENT, dtype=torch.uint8, device="cuda")
    plan = Plan(lib)
    with plan:
        assert lib.glsdet_jpeg_reconstruct(C.byref(da), coef.data_ptr(), qtab.data_ptr(), ws.data_ptr(), ws.numel(), dst.data_ptr(),
                                           3 * 37, 0, None) == 0
    torch.cuda.synchronize()
    assert plan.num_ops == 1 and plan.ops()[0]["name"].startswith("jpeg") and bool((dst == SENT).all())     # recorded, not run

    def load(c, q):
        coef.copy_(_dev(c.reshape(-1)))
        qtab.copy_(_dev(q.reshape(-1).view(np.int16)))
        dst.fill_(SENT)
        torch.cuda.synchronize()

    plan.run()
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), want_a)
    load(cb, qb)
    plan.run()
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), want_b)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        plan.capture(st)
    st.synchronize()
    for c, q, want in ((ca, qa, want_a), (cb, qb, want_b)):
        load(c, q)
        with torch.cuda.stream(st):
            plan.launch(st)
        st.synchronize()
        assert np.array_equal(dst.cpu().numpy(), want)


def test_torch_op_eagerly(lib):
    import glsdet_amd.torch_ops  # noqa: F401
    from glsdet_amd import jpeg as J
    for name in ("ss2-q95-17x33-smooth", "ss1-q100-64x80-noise", "ss0-q30-37x53-noise", "gray-q95-15x31-smooth"):
        d, coef, qtab, rgb = _host(next(c for c in R.CASES if c["name"] == name))
        cd = _dev(coef)
        for qd in (_dev(qtab.view(np.int16)), torch.from_numpy(qtab.copy()).cuda()):               # int16 bits or uint16
            for order, want in ((0, rgb), (1, rgb[:, :, ::-1])):
                y = torch.ops.glsdet.jpeg_reconstruct(cd, qd, J.geometry(d), order)
                torch.cuda.synchronize()
                assert y.dtype == torch.uint8 and y.is_cuda and np.array_equal(y.cpu().numpy(), want)
    with pytest.raises(RuntimeError):
        torch.ops.glsdet.jpeg_reconstruct(cd[:-1], qd, J.geometry(d), 0)
    with pytest.raises(RuntimeError):
        torch.ops.glsdet.jpeg_reconstruct(cd.cpu(), qd.cpu(), J.geometry(d), 0)
    with pytest.raises(RuntimeError):
        torch.ops.glsdet.jpeg_reconstruct(cd, qd, J.geometry(d), 2)


# ------------------------------------------------------------------------------------------------ JpegDecoder
def test_decoder_decode_and_decode_batch_equal_pillow(lib, tmp_path):
    from glsdet_amd.jpeg import JpegDecoder
    from PIL import Image
    dec = JpegDecoder()
    datas = [R.encode(c) for c in R.CASES]
    outs = dec.decode_batch(datas)                          # every size in one go: the staging buffers are reused throughout
    torch.cuda.synchronize()
    for data, t in zip(datas, outs):
        want = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        assert t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous() and np.array_equal(t.cpu().numpy(), want)
    data = datas[-1]
    want = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    path = tmp_path / "a.jpg"
    path.write_bytes(data)
    with open(path, "rb") as f:
        for src in (str(path), path, f):
            assert np.array_equal(dec.decode(src).cpu().numpy(), want)
    assert np.array_equal(dec.decode(data, order="bgr").cpu().numpy(), want[:, :, ::-1])
    # a window of a larger canvas: its row stride is honoured and nothing around it is written
    h, w = want.shape[:2]
    for x0 in (4, 5):
        canvas = torch.full((h + 7, w + 9, 3), SENT, dtype=torch.uint8, device="cuda")
        got = dec.decode(data, out=canvas[3:3 + h, x0:x0 + w])
        torch.cuda.synchronize()
        exp = np.full((h + 7, w + 9, 3), SENT, np.uint8)
        exp[3:3 + h, x0:x0 + w] = want
        assert got.data_ptr() == canvas[3:3 + h, x0:x0 + w].data_ptr() and np.array_equal(canvas.cpu().numpy(), exp)
    with pytest.raises(ValueError):
        dec.decode(data, out=torch.empty(h, w + 1, 3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        dec.decode(data, out=torch.empty(3, h, w, dtype=torch.uint8, device="cuda").permute(1, 2, 0))


def test_drone_preprocessor_on_the_decoder_output_equals_it_on_pillows_array(lib):
    from glsdet_amd.jpeg import JpegDecoder
    from glsdet_amd.preprocess import DronePreprocessor
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(R.picture(203, 117, "smooth", 9)).save(b, "JPEG", subsampling=2, quality=90)
    data = b.getvalue()
    t = JpegDecoder().decode(data)
    pre = DronePreprocessor()
    for letterbox in (False, True):
        a = pre([t], (96, 128), letterbox)
        w = pre([np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))], (96, 128), letterbox)
        assert torch.equal(a, w)


def test_fallback_on_a_progressive_file_and_errors_in_the_entropy_stage(lib):
    from glsdet_amd.jpeg import JpegDecoder, JpegRefused
    from PIL import Image
    rgb = R.picture(37, 53, "smooth", 4)
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", progressive=True, quality=85)
    prog = b.getvalue()
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "PNG")
    png = b.getvalue()
    dec = JpegDecoder(fallback="pillow")
    for data in (prog, png):                                 # a directory of mixed files works
        want = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        assert np.array_equal(dec.decode(data).cpu().numpy(), want)
        assert np.array_equal(dec.decode(data, order="bgr").cpu().numpy(), want[:, :, ::-1])
        canvas = torch.full((60, 40, 3), SENT, dtype=torch.uint8, device="cuda")
        dec.decode(data, out=canvas[2:55, 1:38])
        assert np.array_equal(canvas[2:55, 1:38].cpu().numpy(), want) and int((canvas == SENT).sum()) >= 60 * 40 * 3 - want.size
    with pytest.raises(JpegRefused, match="progressive"):
        JpegDecoder(fallback="raise").decode(prog)
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=85)
    cut = b.getvalue()[:-40]                                 # parses, but the data ends before the last MCU
    for mode in ("pillow", "raise"):
        with pytest.raises(ValueError, match="ends before"):
            JpegDecoder(fallback=mode).decode(cut)
