"""Measures of a segmentation against a ground truth, computed on the device (``medpy.metric``'s binary measures)."""
from . import binary
from .binary import (asd, assd, dc, hd, hd95, jc, positive_predictive_value, precision, ravd, recall, sensitivity, specificity, true_negative_rate,
                     true_positive_rate)

__all__ = ["binary"] + binary.__all__
