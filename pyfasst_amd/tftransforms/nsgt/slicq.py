"""The sliced NSGT (slicq.py, slicing.py, unslicing.py, reblock.py of the
reference) is out of scope: the names exist and refuse."""


class NSGT_sliced(object):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("NSGT_sliced: the sliced transform is not implemented; use NSGT "
                                  "on the whole signal")


class CQ_NSGT_sliced(NSGT_sliced):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("CQ_NSGT_sliced: the sliced transform is not implemented; use "
                                  "CQ_NSGT on the whole signal")
