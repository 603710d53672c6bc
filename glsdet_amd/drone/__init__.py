"""Drop-in root for the reference's `yolox-drone` tree.

Put this directory first on sys.path, the reference's `yolox-drone` root behind it, and the reference's harness
(yolo.py: importlib on a config path string -> `module.YoloBody(num_classes, phi)`; `models.core.utils_bbox`)
resolves to the HIP-backed twins below:

    models/base/yolox.py                              YoloBody            (YOLOX)
    models/block/non_local/yolo_patch_nonlocal_plus.py YoloBody           (YOLOX + GL-fusion neck)
    models/new/yolox6.py, models/lsk/yolox6.py, models/lsk/yolox6_lsk.py   YoloBody (cross-scale head; LSK backbone)
    models/core/utils_bbox.py                         decode_outputs, decode_outputs_cls_sigmoid,
                                                      decode_outputs_no_sigmoid, decode_outputs_no_sigmoid_all,
                                                      decode_outputs_xyxy (one HIP decode, chosen by the harness's
                                                      `decode_mode`), non_max_suppression, yolo_correct_boxes

Every package under models/ extends its __path__ over the same-named directories further down sys.path
(pkgutil.extend_path): a module that has no twin here -- models/core/utils.py, utils_map.py, cocoeval.py, the losses --
is the reference checkout's own file, so yolo.py / yolo_uav.py import unchanged.  Twinned modules win.
"""
