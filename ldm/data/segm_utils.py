"""ldm.data.segm_utils — import path of the reference's style segmenters (segm_utils.py:25-228); the implementation is
upgpt_amd/styles.py, where Segmenter.forward's crops are made on the device (styles.style_crops)."""
from upgpt_amd.inference import clip_normalize, style_names  # noqa: F401
from upgpt_amd.styles import (DEEPFASHION_MM, LIP, DeepfashionMMSegmenter, LipSegmenter, Segmenter, style_boxes,  # noqa: F401
                              style_crops)
