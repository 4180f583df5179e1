"""Drop-in for the three `torch_geometric.utils` names the reference's point decoder imports (scatter, softmax, cumsum),
served by generativedensification_amd.segment.  Nothing else of torch_geometric is provided."""
from generativedensification_amd.segment import cumsum, softmax
from generativedensification_amd.segment import pyg_scatter as scatter

__all__ = ["scatter", "softmax", "cumsum"]
