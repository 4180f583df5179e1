"""Drop-in for the `torch_scatter` names the reference's point decoder uses (lightning/point_decoder/autoencoder.py,
layers/normalization.py, __init__.py), served by the HIP kernels of generativedensification_amd.segment (csrc/segment.hip).
ROCm/HIP tensors only; the envelope and the assumed conventions are listed in INTEGRATION §11."""
from generativedensification_amd.segment import (gather_csr, scatter, scatter_add, scatter_max, scatter_mean, scatter_min,
                                                 scatter_std, scatter_sum, segment_csr, segment_max_csr,
                                                 segment_mean_csr, segment_min_csr, segment_sum_csr)

__all__ = ["segment_csr", "segment_sum_csr", "segment_mean_csr", "segment_min_csr", "segment_max_csr",
           "gather_csr", "scatter", "scatter_sum", "scatter_add", "scatter_mean", "scatter_min", "scatter_max", "scatter_std"]
