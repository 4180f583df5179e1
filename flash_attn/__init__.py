"""Drop-in for the part of the `flash_attn` package the reference's point decoder imports
(lightning/point_decoder/autoencoder.py: `flash_attn.flash_attn_varlen_qkvpacked_func` in every SerializedAttention block),
backed by the MI355X HIP library.  Implementation: generativedensification_amd/attention.py -> libgdr_hip.so (csrc/attn.hip).
Only the packed-QKV functions exist; dropout, masks, windows, softcap and alibi raise NotImplementedError."""
from .flash_attn_interface import flash_attn_qkvpacked_func, flash_attn_varlen_qkvpacked_func  # noqa: F401

__version__ = "2.6.3+gdr.hip"
__all__ = ["flash_attn_qkvpacked_func", "flash_attn_varlen_qkvpacked_func"]
