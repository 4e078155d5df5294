"""
The batch engines: decoded utterances in (numpy arrays or 16-bit frames as stored), results out,
everything in between resident on the device.  One module per feature, as in csrc/capi_*.hip;
_common.py holds what they share.
"""
from ._common import (BEAMFORMER_KINDS, RANK1, Pcm16Frames, channels_and_size,  # noqa: F401
                      compute_vad_masks)
from .enhance import BatchEnhancer  # noqa: F401
from .fixed import FixedBatchBeamformer  # noqa: F401
from .cgmm import CgmmEstimator  # noqa: F401
from .cacgmm import CacgmmEstimator  # noqa: F401
from .dereverb import BatchDereverb, BatchWpd  # noqa: F401
from .auxiva import BatchSeparator  # noqa: F401
from .ssl import BatchLocalizer  # noqa: F401
from .directional import BatchDirectionalFeatures  # noqa: F401
from .spatial import BatchSpatialFeatures  # noqa: F401
from .ns import BatchNoiseSuppressor  # noqa: F401
from .simu import BatchSimulator  # noqa: F401
from .online import BatchOnlineEnhancer  # noqa: F401
from .metric import BatchSiSnr  # noqa: F401
from .rir import BatchRirGenerator  # noqa: F401
from .tfmask import BatchMaskComputer, BatchMaskSeparator, BatchOracleSeparator  # noqa: F401
