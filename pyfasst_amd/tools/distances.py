"""distance / divergence functions (drop-in for tools/distances.py).

A host one-liner in the reference too; the device engines compute the same
quantity on their own planes (simm_reco_error, snmf_run's error vector).
"""
import numpy as np

__all__ = ["ISDistortion"]


def ISDistortion(X, Y):
    """Itakura-Saito divergence between two arrays of the same shape
    (tools/distances.py:9-17)."""
    return np.sum((-np.log(X / Y) + (X / Y) - 1))
