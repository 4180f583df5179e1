"""Drop-in for the `pytorch_msssim` package the reference's training loss and evaluation import
(lightning/loss.py `from pytorch_msssim import MS_SSIM`, evaluation.py `ssim`), backed by the MI355X HIP library.
Implementation: generativedensification_amd/ssim.py -> libgdr_hip.so (csrc/ssim.hip)."""
from generativedensification_amd.ssim import MS_SSIM, SSIM, ms_ssim, ssim  # noqa: F401

__all__ = ["ssim", "ms_ssim", "SSIM", "MS_SSIM"]
