#!/usr/bin/env python
"""scripts/norm_kernel_times.py — kernel times of pe_concat_layer_norm (csrc/norm.hip) with 15 frequencies and with one, at the
same C: the same rows-to-lanes mapping and parent traffic, 1/15 of the sincosf evaluations and fewer output
bytes.  If the kernel reaches the same bytes per second in both, bytes bound it; if the F = 15 kernel reaches fewer, the
difference is what the trig issue costs.  The times come from a kernel trace, so host work is not in them:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o pe -- python scripts/norm_kernel_times.py run
    python scripts/norm_kernel_times.py summarise DIR/pe_kernel_trace.csv

`run` issues, per configuration in CONFIGS order, 40 forwards, then 40 forward + backward pairs (fp32, dense gradient);
`summarise` splits the trace in dispatch order, drops the first calls of each phase and prints median and range per kernel
with the bytes the kernel must move (x, feat read, the padded result written; backward: gradient, x, feat read, dx, dfeat
written) and the rate that gives.
"""
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ((19_200, 4, 256, 15), (19_200, 4, 256, 1), (12_000, 2, 160, 15), (12_000, 2, 160, 1))     # (P, S, C, F)
CALLS = 40


def run():
    import torch

    sys.path.insert(0, ROOT)
    from generativedensification_amd import norm as N

    assert torch.cuda.is_available(), "norm_kernel_times needs the GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    for p, s, c, f in CONFIGS:
        g = torch.Generator().manual_seed(p + f)
        x = (0.004 * torch.tanh(torch.randn(p * s, 3, generator=g))).to(dev)
        feat = torch.randn(p, c, generator=g).to(dev)
        freq = (2.0 ** torch.arange(f)).to(dev)
        gout = torch.randn(p * s, 6 * f + c, generator=g).to(dev)
        for _ in range(CALLS):
            N.pe_concat_layer_norm(x, feat, freq, s)
        torch.cuda.synchronize()
        x.requires_grad_(True)
        feat.requires_grad_(True)
        for _ in range(CALLS):
            torch.autograd.grad(N.pe_concat_layer_norm(x, feat, freq, s), (x, feat), gout)
        torch.cuda.synchronize()


def summarise(path):
    rows = [r for r in csv.DictReader(open(path)) if "pe_fwd_kernel" in r["Kernel_Name"] or "pe_bwd_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    assert len(rows) == 3 * CALLS * len(CONFIGS), f"{len(rows)} pe kernels in the trace, expected {3 * CALLS * len(CONFIGS)}"
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3      # noqa: E731
    for i, (p, s, c, f) in enumerate(CONFIGS):
        chunk = rows[i * 3 * CALLS:(i + 1) * 3 * CALLS]
        fwd = [us(r) for r in chunk if "pe_fwd_kernel" in r["Kernel_Name"]][10:]
        bwd = [us(r) for r in chunk if "pe_bwd_kernel" in r["Kernel_Name"]][5:]
        w = 6 * f + c
        wp = (w + 7) // 8 * 8
        for name, t, nbytes in (("forward", fwd, p * s * 12 + p * c * 4 + p * s * wp * 4),
                                ("backward", bwd, p * s * w * 4 + 2 * p * s * 12 + 2 * p * c * 4)):
            m = statistics.median(t)
            print(f"P {p} S {s} C {c} F {f} {name}: {m:.2f} us ({min(t):.2f}-{max(t):.2f}), {nbytes / 1e6:.1f} MB, "
                  f"{nbytes / m / 1e6:.2f} TB/s")


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "summarise":
        summarise(sys.argv[2])
    else:
        sys.exit(__doc__)
