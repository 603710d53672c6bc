# Fine detector of UFPMP-Det on the ResNeXt-101 32x4d backbone (backbones/resnext.py:109-154): MPDet = ResNeXt + FPN +
# MPHead.  C2..C5 keep the ResNet widths, so neck and head are those of mp_det_res50.py.
_base_ = ['./mp_det_res50.py']
model = dict(
    backbone=dict(
        _delete_=True,
        type='ResNeXt', depth=101, groups=32, base_width=4, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
        norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, style='pytorch'))
