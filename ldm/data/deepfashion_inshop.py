"""ldm.data.deepfashion_inshop — import path of the reference's test-split datasets (deepfashion_inshop.py:21-362), the
`target` of every UPGPT model config's data section; the implementation is upgpt_amd/data.py, where the batch is
assembled on the device."""
from upgpt_amd.data import (DeepFashionPair, DeepFashionSample, convert_fname, get_name, list_subdirectories,  # noqa: F401
                            style_names)
