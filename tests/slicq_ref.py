"""NumPy restatement of the sliced NSGT (test infrastructure only): the sliced
planner (Blackman-Harris windows on even positions), the slicing into
Tukey-windowed half-overlapping slices, the per-slice transform of
tests/nsgt_ref.py, the per-slice band rotation and the unslicing.
tests/golden/slicq_*.npz pins it to the reference; the GPU tests compare the
device against it live.
"""
import warnings

import numpy as np

import nsgt_ref as NR

TIGHT = 1e-9   # the project's FP64 bound, relative to the largest magnitude

# case -> what to build; mirrors tests/golden/make_golden_slicq.py
SMALL = dict(fmin=200, fmax=3500, bins=4, fs=8000, sl_len=1024, tr_area=128, real=True, L=3001)
BIG = dict(sl_len=20000, tr_area=5000, fs=44100, real=True, L=100000, big=True)
CASES = {
    "small": SMALL,
    "complex": dict(SMALL, real=False),
    "matrix": dict(SMALL, matrixform=True),
    "recwnd": dict(SMALL, recwnd=True),
    "qvar": dict(SMALL, Qvar=2),
    "tiny": dict(fmin=300, fmax=3800, bins=3, fs=8000, sl_len=512, tr_area=64, real=True, L=2500),
    "big6": dict(BIG, fmin=80, fmax=18200, bins=6),
    "big2": dict(BIG, fmin=100, fmax=18200, bins=2),
}
SMALL_CASES = [n for n in sorted(CASES) if not CASES[n].get("big")]
BIG_CASES = [n for n in sorted(CASES) if CASES[n].get("big")]
BIG_STORED = (0, 1, -1)   # the slices a big case's fixture holds
OPTIONS = ("real", "recwnd", "matrixform", "Qvar")


def signal(name):
    rs = np.random.RandomState(sum(map(ord, name)) + 7)
    return rs.randn(CASES[name]["L"])


def options(c):
    return dict((k, c[k]) for k in OPTIONS if k in c)


# ----------------------------------------------------------------- planning
def blackharr(n):
    period = (n // 2) * 2
    k = np.arange(n)
    bh = (0.35872 - 0.48832 * np.cos(k * (2 * np.pi / period))
          + 0.14128 * np.cos(k * (4 * np.pi / period)) - 0.01168 * np.cos(k * (6 * np.pi / period)))
    return np.hstack((bh[-n // 2:], bh[:-n // 2]))


def windows_sliced(f, q, sr, sl_len, min_win=16, Qvar=1):
    """g, rfbas, M of the sliced planner."""
    nf = sr / 2.
    lim = np.argmax(f > 0)
    if lim != 0:
        f, q = f[lim:], q[lim:]
    lim = np.argmax(f >= nf)
    if lim != 0:
        f, q = f[:lim], q[:lim]
    lbas = len(f)
    frqs = np.concatenate(((0.,), f, (nf,)))
    fbas = np.concatenate((frqs, sr - frqs[-2:0:-1]))
    fbas *= float(sl_len) / sr
    M = np.zeros(fbas.shape, float)
    M[0] = 2 * fbas[1]
    M[1] = fbas[1] / q[0]
    for k in list(range(2, lbas)) + [lbas + 1]:
        M[k] = fbas[k + 1] - fbas[k - 1]
    M[lbas] = fbas[lbas] / q[lbas - 1]
    M[lbas + 2:2 * (lbas + 1)] = M[lbas:0:-1]
    M *= Qvar / 4.
    M = np.round(M).astype(int)
    M *= 4
    M = np.maximum(M, min_win)
    g = [blackharr(m) for m in M]
    for kk in (1, lbas + 2):
        if M[kk - 1] > M[kk]:
            g[kk - 1] = np.ones(M[kk - 1])
            lo = M[kk - 1] // 2 - M[kk] // 2
            g[kk - 1][lo:lo + M[kk]] = NR.hann(M[kk])
    return g, np.round(fbas / 2.).astype(int) * 2, M


def tukey(sl_len, tr_area):
    hhop, htr = sl_len // 4, tr_area // 2
    w = NR.hann(2 * tr_area)
    tw = np.zeros(sl_len)
    tw[hhop - htr:hhop + htr] = w[tr_area:]
    tw[hhop + htr:3 * hhop - htr] = 1
    tw[3 * hhop - htr:3 * hhop + htr] = w[:tr_area]
    return tw


def synthesis(sl_len, tr_area):
    hhop, htr = sl_len // 4, tr_area // 2
    tr2 = min(2 * hhop - tr_area, 2 * tr_area)
    htr2 = tr2 // 2
    hw = NR.hann(tr2)
    tw = np.zeros(sl_len)
    tw[hhop - htr - htr2:hhop - htr] = hw[htr2:]
    tw[hhop - htr:3 * hhop + htr] = 1
    tw[3 * hhop + htr:3 * hhop + htr + htr2] = hw[:htr2]
    return tw


def quarter(i, k):
    """Where quarter i of a slice of parity k sits inside the slice."""
    return (i + 3 - 2 * k) % 4


class SlicedPlan(NR.Plan):
    """forward / backward (inherited) are the per-slice transforms without
    rotation; forward_stream / backward_stream the whole sliced transform."""

    def __init__(self, f, q, fs, sl_len, tr_area, real=False, recwnd=False, matrixform=False,
                 reducedform=0, min_win=16, Qvar=1):
        self.Ls, self.real, self.reducedform = sl_len, real, reducedform
        self.sl_len, self.tr_area, self.hhop, self.recwnd = sl_len, tr_area, sl_len // 4, recwnd
        self.g, self.rfbas, self.M = windows_sliced(f, q, fs, sl_len, min_win, Qvar)
        if matrixform:
            nb = len(self.M)
            self.M[:] = (self.M[reducedform:nb // 2 + 1 - reducedform] if reducedform
                         else self.M).max()
        self.wins, self.nn = NR.win_ranges(self.g, self.rfbas, sl_len)
        self.gd = NR.duals(self.g, self.wins, self.nn, self.M)

    def nslices(self, L):
        return (-(-L // self.hhop) + 1) // 2 + 1

    def slices(self, x):
        """The Tukey-windowed slices of x, quarters in the rotated order."""
        hhop, N = self.hhop, self.nslices(len(x))
        stream = np.zeros((2 * N + 2) * hhop)
        stream[2 * hhop:2 * hhop + len(x)] = x
        tw = tukey(self.sl_len, self.tr_area)
        out = []
        for s in range(N):
            sl = np.empty(self.sl_len)
            for i in range(4):
                p = quarter(i, s % 2)
                sl[p * hhop:(p + 1) * hhop] = (stream[(2 * s + i) * hhop:(2 * s + i + 1) * hhop]
                                               * tw[i * hhop:(i + 1) * hhop])
            out.append(sl)
        return out

    @staticmethod
    def rotate(c, s, fwd):
        """Band rotation of slice s: out[j] = c[j + shift], shift 3M/4 on even
        slices forward (M/4 backward), the other one on odd slices."""
        out = []
        for b in c:
            m = len(b)
            shift = 3 * m // 4 if (s % 2 == 0) == fwd else m // 4
            out.append(np.concatenate((b[shift:], b[:shift])))
        return out

    def forward_stream(self, x):
        return [self.rotate(self.forward(sl), s, True) for s, sl in enumerate(self.slices(x))]

    def unslice(self, frec):
        """Overlap-add of the slices' quarters, older slice first: the stream
        without its two leading padding blocks, 2 hhop samples per slice."""
        hhop, N = self.hhop, len(frec)
        tw = synthesis(self.sl_len, self.tr_area) if self.recwnd else None
        out = np.zeros((2 * N + 2) * hhop, dtype=float if self.real else complex)
        for s, fr in enumerate(frec):
            for i in range(4):
                p = quarter(i, s % 2)
                part = fr[p * hhop:(p + 1) * hhop]
                if tw is not None:
                    part = part * tw[i * hhop:(i + 1) * hhop]
                out[(2 * s + i) * hhop:(2 * s + i + 1) * hhop] += part
        return out[2 * hhop:]

    def backward_stream(self, cs):
        return self.unslice([self.backward(self.rotate(c, s, False)) for s, c in enumerate(cs)])


_plans = {}


def plan_of(name):
    if name not in _plans:
        c = CASES[name]
        f, q = NR.oct_scale(c["fmin"], c["fmax"], c["bins"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _plans[name] = SlicedPlan(f, q, c["fs"], c["sl_len"], c["tr_area"], **options(c))
    return _plans[name]


_streams = {}


def reference_of(name):
    """(signal, the restatement's coefficients per slice, its reconstruction),
    computed once per case and shared: do not modify."""
    if name not in _streams:
        p, x = plan_of(name), signal(name)
        cs = p.forward_stream(x)
        _streams[name] = (x, cs, p.backward_stream(cs))
    return _streams[name]
