# Fine detector of UFPMP-Det on the ResNeXt-101 64x4d backbone: mp_det_x101_32x4d.py with 64 groups.
_base_ = ['./mp_det_x101_32x4d.py']
model = dict(backbone=dict(groups=64))
