"""The plug-in recipe of INTEGRATION.md section 1 on the reference's own harness files: with `glsdet_amd/drone` first on
sys.path and the reference's `yolox-drone` root behind it, `yolo.py` / `yolo_uav.py` import UNCHANGED -- the twinned
modules (`models.core.utils_bbox`, the `YoloBody` configs) come from this repository, everything else
(`models.core.utils`, ...) from the checkout -- and `YOLO(decode_mode=...)` picks the twin's decode function.

CPU only; each test that needs the reference checkout skips where it is not mounted.  No file of the checkout is
edited or copied.  The last tests need no checkout: the recorded outputs of the reference's five decode functions
(tests/golden/decode_modes_golden.npz, written by tests/golden/make_decode_golden.py) against the float64 restatement
the GPU tests use, and the host-side refusal of a bad sigmoid mask."""
import importlib
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from tests import decode_reference as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = os.path.join(ROOT, "glsdet_amd", "drone")
REF = "/root/reference/yolox-drone"
HARNESS = ["yolo.py", "yolo_uav.py", "tools/uav_tools/yolo_uav.py"]
DECODE_NAMES = ("decode_outputs", "decode_outputs_no_sigmoid", "decode_outputs_no_sigmoid_all", "decode_outputs_cls_sigmoid")


def _is_models(name):
    return name == "models" or name.startswith("models.")


@pytest.fixture()
def harness_path():
    """drop-in root first, reference root second; `models*` of other tests out of sys.modules and back afterwards"""
    if not os.path.isdir(REF):
        pytest.skip("the reference checkout is not mounted here")
    saved = {k: v for k, v in sys.modules.items() if _is_models(k)}
    for k in saved:
        del sys.modules[k]
    old_path = list(sys.path)
    sys.path[:0] = [DROP, REF]
    importlib.invalidate_caches()
    yield
    sys.path[:] = old_path
    for k in [k for k in sys.modules if _is_models(k)]:
        del sys.modules[k]
    sys.modules.update(saved)


def _exec(rel):
    spec = importlib.util.spec_from_file_location("ref_harness_" + rel[:-3].replace("/", "_"), os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                       # module level: imports + the YOLO class; nothing is run
    return mod


@pytest.mark.parametrize("rel", HARNESS)
def test_reference_harness_imports_unchanged_behind_the_drop_in_root(harness_path, rel):
    mod = _exec(rel)
    twin = importlib.import_module("models.core.utils_bbox")
    assert os.path.realpath(twin.__file__) == os.path.realpath(os.path.join(DROP, "models", "core", "utils_bbox.py"))
    for name in DECODE_NAMES + ("non_max_suppression",):
        fn = getattr(mod, name)
        assert fn.__module__ == "models.core.utils_bbox" and fn is getattr(twin, name), name
    assert callable(twin.decode_outputs_xyxy)
    # not twinned: the checkout's own file
    utils = importlib.import_module("models.core.utils")
    assert os.path.realpath(utils.__file__) == os.path.realpath(os.path.join(REF, "models", "core", "utils.py"))
    for name in ("cvtColor", "get_classes", "preprocess_input", "resize_image"):
        assert getattr(mod, name) is getattr(utils, name), name
    assert importlib.util.find_spec("models.core.utils_map").origin.startswith(REF)      # located, not run (it needs cv2)
    # twinned detector configs still win over the checkout's
    for cfg in ("models.base.yolox", "models.block.non_local.yolo_patch_nonlocal_plus"):
        assert os.path.realpath(importlib.import_module(cfg).__file__).startswith(os.path.realpath(DROP)), cfg
    assert hasattr(mod, "YOLO")


@pytest.mark.parametrize("decode_mode", sorted(D.HARNESS_MODES))
def test_reference_yolo_constructs_on_the_twin_for_every_decode_mode(harness_path, tmp_path, decode_mode):
    """yolo.py:71-111 as shipped: decode_mode -> decode_func, get_classes (checkout), importlib on the config path ->
    the twin's YoloBody, torch.load + load_state_dict, eval.  cuda=False: nothing touches a GPU."""
    mod = _exec("yolo.py")
    twin = importlib.import_module("models.core.utils_bbox")
    body = importlib.import_module("models.base.yolox")
    names = ["class%d" % i for i in range(10)]
    (tmp_path / "classes.txt").write_text("\n".join(names) + "\n")
    torch.save(body.YoloBody(10, "s").state_dict(), tmp_path / "twin.pth")
    yolo = mod.YOLO(cuda=False, config_path="models/base/yolox.py", phi="s", model_path=str(tmp_path / "twin.pth"),
                    classes_path=str(tmp_path / "classes.txt"), decode_mode=decode_mode)
    assert yolo.decode_func is getattr(twin, D.HARNESS_MODES[decode_mode])
    assert yolo.num_classes == 10 and yolo.class_names == names
    assert type(yolo.net) is body.YoloBody and not yolo.net.training
    from glsdet_amd.drone.body import HipYoloBody
    assert isinstance(yolo.net, HipYoloBody)


def test_harness_names_and_twin_share_one_mask_table():
    from glsdet_amd.engine import DECODE_MODES
    assert DECODE_MODES == {"default": 3, "obj_sigmoid": 1, "no_sigmoid": 0, "cls_sigmoid": 2}
    for mode, fn in D.HARNESS_MODES.items():
        assert D.VARIANTS[fn] == (0, DECODE_MODES[mode])


def test_float64_restatement_reproduces_the_reference_golden():
    """The five recorded float32 outputs of the reference against decode_f64.  Measured against the live reference:
    max |err| / (|x| + 1) = 8.6e-8 for the four normalised variants, 9.0e-7 for xyxy; asserted at the decode bound."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "decode_modes_golden.npz"))
    levels = [torch.from_numpy(g["level%d" % l]) for l in range(3)]
    in_h, in_w = (int(v) for v in g["input_shape"])
    nc = int(g["num_classes"])
    assert in_h != in_w and any(in_h / x.shape[2] != in_w / x.shape[3] for x in levels)      # pins stride = in_h / h
    assert float(torch.cat([x[:, 2:4].flatten() for x in levels]).abs().max()) == 20.0
    assert set("ref/" + k for k in D.VARIANTS) <= set(g.files)
    for name, (mode, mask) in D.VARIANTS.items():
        want = D.decode_f64(levels, nc, in_h, in_w, None, mode, None, mask)
        err = D.rel_err(g["ref/" + name], want)
        print("%s: reference float32 vs float64 restatement %.3e" % (name, err))
        assert g["ref/" + name].dtype == np.float32 and err <= D.BOUND, (name, err)
    # what the mask leaves alone is the input logit itself
    raw = torch.cat([x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1]) for x in levels], 1).numpy()
    assert np.array_equal(g["ref/decode_outputs_no_sigmoid_all"][..., 4:].view(np.uint32), raw[..., 4:].view(np.uint32))
    assert np.array_equal(g["ref/decode_outputs_no_sigmoid"][..., 5:].view(np.uint32), raw[..., 5:].view(np.uint32))
    assert np.array_equal(g["ref/decode_outputs_cls_sigmoid"][..., 4].view(np.uint32), raw[..., 4].view(np.uint32))


def _view(n, h, w, c, base=0x10000):
    from glsdet_amd import _lib
    v = _lib.View()
    v.base, v.n, v.h, v.w, v.c, v.dtype = base, n, h, w, c, _lib.F32
    v.sw, v.sh, v.sn = c, w * c, h * w * c
    v.alloc_lo, v.alloc_hi = base, base + n * h * w * c * 4
    return v


@pytest.mark.parametrize("mask", [-1, 4])
def test_decode_ex_refuses_a_bad_sigmoid_mask_before_any_launch(mask):
    """host-side validation (the pointers are never dereferenced: runs without a GPU)"""
    import __graft_entry__ as g
    g.build()
    from glsdet_amd import _lib
    lib = _lib.load()
    lv = (_lib.View * 1)(_view(2, 4, 4, 16))
    rc = lib.glsdet_yolox_decode_ex(lv, 1, 10, 32, 32, None, 0, mask, 0x900000, 2 * 16 * 15, None, None)
    msg = lib.glsdet_last_error().decode()
    assert rc == -1 and "yolox_decode" in msg and "sigmoid_mask" in msg, (rc, msg)
    # the same call is refused for its box format as well, under the same name
    assert lib.glsdet_yolox_decode_ex(lv, 1, 10, 32, 32, None, 2, 3, 0x900000, 2 * 16 * 15, None, None) == -1
    assert "yolox_decode" in lib.glsdet_last_error().decode()
