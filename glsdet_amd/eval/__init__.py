"""Evaluation side of the detection path: result formats, bbox COCOeval, VOC-style mAP."""
from .coco import COCO
from .cocoeval import COCOeval, Params
from .results import (VISDRONE_CLASSES, ResultMerger, coco_records, detection_line, parse_detection_results,
                      parse_per_class, write_detection_results)
from .voc import VocEval, get_map

__all__ = ["COCO", "COCOeval", "Params", "VISDRONE_CLASSES", "VocEval", "get_map", "ResultMerger", "coco_records", "detection_line",
           "parse_detection_results", "parse_per_class", "write_detection_results"]
