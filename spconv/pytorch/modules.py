"""spconv.pytorch.modules: the module test of the reference's PointSequential.forward."""
from generativedensification_amd.sparse_conv import SparseModule, is_spconv_module

__all__ = ["SparseModule", "is_spconv_module"]
