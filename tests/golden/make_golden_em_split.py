"""Write tests/golden/em_split.npz, or with --more tests/golden/em_split_more.npz:
what the runs of tests/em_split_cases.py give on an MI355X.

Run on the commit before the move it guards (em_split.npz: before the E-step
left fasst_em.hip; em_split_more.npz: before the mixing, renormalisation and
spectral phases did), so the file records what the parent library computed:

    python tests/golden/make_golden_em_split.py [--more] [out.npz]

em_split.npz: the ten GEM runs CASES.  em_split_more.npz: the GEM runs k and l,
the stand-alone ABI sequence m, and for every GEM run a - l the timed launches
per kernel slot of a run with profiling on, whose parameters must equal the
unprofiled run's bit for bit.

Every case runs twice; a case whose two runs are not bit-equal cannot carry a
tolerance of 0 and is left out (named on stdout).  The results depend on the
device's CU count through configure_model's schedules: generate and check on
the same machine type.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import em_split_cases as cases  # noqa: E402


def same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


def twice(label, fn, report):
    """fn()'s arrays if two calls give them bit for bit, else None."""
    a, b = fn(), fn()
    ok = same(a, b)
    finite = all(np.isfinite(v).all() for v in a.values())
    print("case %s: %s, %s" % (label, "bit-repeatable" if ok else "NOT bit-repeatable: left out",
                               report(a)), "" if finite else "NOT FINITE")
    return a if ok else None


def gem(name, keep):
    got = twice(name, lambda: cases.run(name), lambda a: "loglik %s, (done, mask) %s" % (
        a["%s_loglik" % name], a["%s_done_mask" % name]))
    if got:
        keep.update(got)
    return got


if __name__ == "__main__":
    args = sys.argv[1:]
    more = "--more" in args
    args = [a for a in args if a != "--more"]
    out = args[0] if args else os.path.join(HERE, "em_split_more.npz" if more else "em_split.npz")
    keep = {}
    if not more:
        for name in cases.CASES:
            gem(name, keep)
    else:
        plain = {name: cases.run(name) for name in cases.CASES}
        for name in ("k", "l"):
            plain[name] = gem(name, keep)
        got = twice("m", cases.run_abi, lambda a: "masks %s" % a["m_masks"])
        if got:
            keep.update(got)
        for name, ref in plain.items():
            key = "%s_launches" % name
            got = twice(name + " profiled", lambda: cases.run(name, profile=True), lambda a: "launches %s" % a[key])
            if got and ref and same({k: v for k, v in got.items() if k != key}, ref):
                keep[key] = got[key]
            else:
                print("case %s: the profiled run's parameters differ from the unprofiled run's: left out" % name)
    np.savez_compressed(out, **keep)
    print("wrote %s: %d arrays, %d bytes" % (out, len(keep), os.path.getsize(out)))
