"""`import spconv.pytorch as spconv`: exactly the names the reference uses (lightning/point_decoder/utils/structure.py,
utils/modules.py, autoencoder.py)."""
from generativedensification_amd.sparse_conv import SparseConvTensor, SparseModule, SubMConv3d

from . import modules

__all__ = ["SparseConvTensor", "SubMConv3d", "SparseModule", "modules"]
