"""The reference's spatial package on the GPU: steering vectors and
directivity diagrams (spatial/steering_vectors.py, spatial/dirdiag.py)."""
