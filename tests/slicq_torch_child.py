"""Child process of tests/test_gpu_slicq.py: the torch-tensor route of the
sliced NSGT.  It runs in a process of its own because torch must have
initialised the GPU before the library's first device call.  Prints one JSON
line: per case, what was checked.  `stereo` is `small` on two channels, three
slices a call.
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

CASES = {"small": ("small", {}), "complex": ("complex", {}), "recwnd": ("recwnd", {}),
         "stereo": ("small", dict(multichannel=True, slices_per_call=3))}


def main():
    dev = torch.device('cuda', 0)
    torch.zeros(1, device=dev)                       # torch initialises the GPU first
    import slicq_ref as SR
    from pyfasst_amd.tftransforms.slicq import CQ_NSGT_sliced
    out = {}
    for label, (name, over) in CASES.items():
        c = SR.CASES[name]
        multi = over.get("multichannel", False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t = CQ_NSGT_sliced(c["fmin"], c["fmax"], c["bins"], c["sl_len"], c["tr_area"], c["fs"],
                               **dict(SR.options(c), **over))
        x = SR.signal(name)
        if multi:
            x = np.array([x, x[::-1] * 0.5])
        host_c = list(t.forward((x,)))               # the NumPy route
        host_y = np.concatenate(list(t.backward(host_c)), axis=-1)
        if multi:
            flat = np.array([[np.concatenate(ch) for ch in it] for it in host_c])
        else:
            flat = np.array([np.concatenate(it) for it in host_c])
        tx = torch.as_tensor(x, device=dev)
        tc, off = t.forward(tx)
        ty = t.backward((tc, off))
        lens = [len(b) for b in (host_c[0][0] if multi else host_c[0])]
        r = {"tensor_out": bool(torch.is_tensor(tc) and tc.device == dev
                                and tc.dtype == torch.complex128 and torch.is_tensor(ty)
                                and ty.device == dev
                                and ty.dtype == (torch.float64 if c["real"] else torch.complex128)),
             "shapes_ok": bool(np.array_equal(np.diff(off), lens) and tc.shape[-1] == off[-1]
                               and tuple(tc.shape) == flat.shape
                               and tuple(ty.shape) == host_y.shape
                               and ty.shape[-1] == 2 * t.hhop * len(host_c)),
             "forward_bit_equal": bool(np.array_equal(tc.cpu().numpy(), flat)),
             "backward_bit_equal": bool(np.array_equal(ty.cpu().numpy(), host_y))}
        # a producer's pending work on the current stream is waited for
        y2 = t.backward(t.forward(tx * 2.0)[0])
        L = x.shape[-1]
        r["scaled"] = float(np.max(np.abs(y2.cpu().numpy()[..., :L] - 2.0 * x)) / np.max(np.abs(x)))
        out[label] = r
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
