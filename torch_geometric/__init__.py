"""Drop-in for `torch_geometric`: only `torch_geometric.utils.{scatter, softmax, cumsum}`, what the reference's point decoder
imports (see torch_geometric/utils/__init__.py)."""
from . import utils
from .utils import cumsum, scatter, softmax

__all__ = ["scatter", "softmax", "cumsum"]
