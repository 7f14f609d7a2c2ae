"""Transform registry (tftransforms/tft.py:74-81): the abbreviated names
SeparateLeadProcess and FASST use to build their time-frequency transforms.
STFT, CQT and MinQT run on the GPU; the NSGT ('nsgmqt') is outside the
GPU path."""
from .minqt import CQTransfo, MinQTransfo, sqrt_blackmanharris  # noqa: F401
from .stft import STFT  # noqa: F401


class TFTransform(object):
    """Base class of the time-frequency transforms (tft.py:12-72): a subclass
    implements `computeTransform`, which stores its result in `transfo`, and
    `invertTransform`, which inverts what `transfo` holds.  It accepts every
    transform's constructor arguments and ignores them."""
    transformname = 'dummy'
    transfo = None

    def __init__(self, fmin=25, fmax=1000, bins=12, fs=44100, q=1, atomHopFactor=0.25,
                 thresh=0.0005, winFunc=None, perfRast=0, cqtkernel=None, lowPassCoeffs=None,
                 data=None, verbose=0, **kwargs):
        pass

    def computeTransform(self, data):
        pass

    def invertTransform(self):
        pass


tftransforms = {
    'stftold': TFTransform,
    'stft': STFT,
    'mqt': MinQTransfo,
    'minqt': MinQTransfo,
    'cqt': CQTransfo}
"""A convenience dictionary, with abbreviated names for the transforms."""
