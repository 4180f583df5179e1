"""Drop-in for the part of `spconv` 2.x that the reference's point decoder touches (`import spconv.pytorch as spconv`):
SparseConvTensor, SubMConv3d, SparseModule and modules.is_spconv_module, served by the HIP kernels of
generativedensification_amd.sparse_conv.  Strided / transposed sparse convolution and SparseSequential are not provided."""
from . import pytorch  # noqa: F401

__all__ = ["pytorch"]
