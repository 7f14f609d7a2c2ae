"""The sliced NSGT lives in pyfasst_amd.tftransforms.slicq; the names of this
package refuse and point there."""


class NSGT_sliced(object):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("nsgt.NSGT_sliced refuses: the sliced transform is "
                                  "pyfasst_amd.tftransforms.slicq.NSGT_sliced")


class CQ_NSGT_sliced(NSGT_sliced):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("nsgt.CQ_NSGT_sliced refuses: the sliced transform is "
                                  "pyfasst_amd.tftransforms.slicq.CQ_NSGT_sliced")
