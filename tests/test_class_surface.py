"""Every method of the reference's FASST, MultiChanNMFInst_FASST and
MultiChanNMFConv classes (tests/golden/fasst_class_surface.txt: one
`Class.method` per line, each class with its inherited ones) exists on the
class of the same name in pyfasst_amd.audioModel, so a script that changes
only its import finds them.  CPU only: nothing is called."""
import os

import pytest

from helpers import GOLDEN

NAMES = [l.strip() for l in open(os.path.join(GOLDEN, "fasst_class_surface.txt")) if l.strip()]


def test_list_covers_the_three_classes():
    assert {n.split('.')[0] for n in NAMES} == {'FASST', 'MultiChanNMFInst_FASST',
                                                'MultiChanNMFConv'}
    assert len(NAMES) == len(set(NAMES))


@pytest.mark.parametrize("name", NAMES)
def test_method_exists(name):
    import pyfasst_amd.audioModel as am
    cls, meth = name.split('.')
    assert callable(getattr(getattr(am, cls), meth, None)), name
