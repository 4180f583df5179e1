"""CPU: the float64 restatement of the segment reductions (tests/scatter_ref.py) against torch's own CPU operators, the
surface of the torch_scatter / torch_geometric drop-ins against what the reference calls (tests/golden/scatter_surface.json),
the refusals that need no GPU, and the workspace size of the kernels."""
import importlib
import inspect
import json
import os

import numpy as np
import pytest
import torch

import scatter_cases as SC
import scatter_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SURFACE = json.load(open(os.path.join(HERE, "golden", "scatter_surface.json")))


@pytest.mark.parametrize("layout", list(SC.layouts(32)))
def test_restatement_agrees_with_torch_on_the_cpu(layout):
    n, ptr = SC.layouts(32)[layout]
    s = len(ptr) - 1
    src = SC.integers((n, 5), seed=n + 1)
    lengths = torch.from_numpy(np.diff(ptr))
    inside = torch.from_numpy(src[int(ptr[0]):int(ptr[-1])])
    if s == 0:       # torch.segment_reduce takes no empty lengths: only the shapes
        assert all(R.segment_csr(src, ptr, op)[0].shape == (0, 5) for op in ("sum", "mean", "min", "max"))
        assert R.gather_csr(src[:0], ptr).shape == (0, 5) and R.cumsum(np.zeros(0, dtype=np.int64)).tolist() == [0]
        return
    for op in ("sum", "mean", "min", "max"):
        out, arg = R.segment_csr(src, ptr, op)
        want = torch.segment_reduce(inside, op, lengths=lengths, axis=0)
        want[lengths == 0] = 0          # torch gives an empty segment the identity of the reduction or nan: 0 here
        assert out.shape == (s, 5) and np.array_equal(out, want.numpy()), op
        if arg is not None:
            for i in range(s):
                a, b = int(ptr[i]), int(ptr[i + 1])
                if b > a:       # the value at arg is the extreme, and no earlier row of the segment holds it
                    assert (np.take_along_axis(src, arg[i][None], 0)[0] == out[i]).all()
                    assert all((src[a:arg[i][c], c] != out[i][c]).all() for c in range(5))
                else:
                    assert (arg[i] == n).all() and (out[i] == 0).all()
    # the index route on the same rows: index_add_ / index_reduce_
    index = np.repeat(np.arange(s), np.diff(ptr))
    rows = src[int(ptr[0]):int(ptr[-1])]
    shuffle = np.random.default_rng(1).permutation(len(index))
    got = R.scatter(rows[shuffle], index[shuffle], s, "sum")[0]
    want = torch.zeros(s, 5, dtype=torch.float64).index_add_(0, torch.from_numpy(index[shuffle]), torch.from_numpy(rows[shuffle]))
    assert np.array_equal(got, want.numpy())
    got, arg = R.scatter(rows[shuffle], index[shuffle], s, "max")
    want = torch.zeros(s, 5, dtype=torch.float64).index_reduce_(0, torch.from_numpy(index[shuffle]), torch.from_numpy(rows[shuffle]),
                                                                "amax", include_self=False)
    assert np.array_equal(got, want.numpy())
    # gather, the gradients in closed form against autograd of the torch composition, cumsum
    g = SC.integers((s, 5), seed=9)
    assert np.array_equal(R.gather_csr(g, ptr)[int(ptr[0]):], torch.from_numpy(g).repeat_interleave(lengths, dim=0).numpy())
    x = torch.from_numpy(src).requires_grad_(True)
    torch.segment_reduce(x[int(ptr[0]):int(ptr[-1])], "mean", lengths=lengths, axis=0, initial=0.0).backward(torch.from_numpy(g))
    assert np.allclose(R.segment_csr_grad(src.shape, ptr, "mean", g), x.grad.numpy(), rtol=0, atol=1e-15)
    assert np.array_equal(R.cumsum(np.diff(ptr)), np.asarray(ptr) - ptr[0])


def test_restatement_of_softmax_and_std_agrees_with_torch():
    rng = np.random.default_rng(2)
    sizes = [5, 1, 9]
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    x = rng.standard_normal((15, 2))
    y, index = R.softmax_ptr(x, ptr)
    t = torch.from_numpy(x).requires_grad_(True)
    want = torch.cat([torch.softmax(t[ptr[i]:ptr[i + 1]], 0) for i in range(3)])
    assert np.allclose(y, want.detach().numpy(), rtol=0, atol=1e-15)
    g = rng.standard_normal((15, 2))
    want.backward(torch.from_numpy(g))
    assert np.allclose(R.softmax_grad(y, g, index, 3), t.grad.numpy(), rtol=0, atol=1e-14)
    std = R.scatter_std(x, index, 4)
    for i in range(3):
        rows = torch.from_numpy(x[ptr[i]:ptr[i + 1]])
        want = rows.std(0, unbiased=True) if sizes[i] > 1 else torch.zeros(2, dtype=torch.float64)
        assert np.allclose(std[i], want.numpy(), rtol=2e-6, atol=0)      # (the 1e-6 of the denominator)
    assert (std[3] == 0).all()


def test_number_format_helpers():
    a = torch.tensor([1.0, -1.0, 0.0, 2.0], dtype=torch.bfloat16)
    b = torch.tensor([1.0078125, -1.0078125, -0.0, 2.0], dtype=torch.bfloat16)
    assert R.ulp_distance(a, b).tolist() == [1, 1, 0, 0]
    assert R.half_ulp(1.0, torch.float32) == 2.0 ** -24 and R.half_ulp(3.0, torch.float16) == 2.0 ** -10
    assert R.half_ulp(0.0, torch.float16) == 2.0 ** -25


def test_drop_ins_export_the_names_and_keywords_the_reference_uses():
    import torch_geometric
    import torch_geometric.utils
    import torch_scatter

    assert sorted(torch_geometric.utils.__all__) == sorted(torch_geometric.__all__) == ["cumsum", "scatter", "softmax"]
    assert not hasattr(torch_scatter, "segment_add_csr")        # only the names the reference can reach
    for name in ("segment_csr", "segment_sum_csr", "segment_mean_csr", "segment_min_csr", "segment_max_csr", "gather_csr",
                 "scatter", "scatter_sum", "scatter_add", "scatter_mean", "scatter_min", "scatter_max", "scatter_std"):
        assert name in torch_scatter.__all__ and callable(getattr(torch_scatter, name))
    seen = set()
    for module, rec in SURFACE.items():
        for package, names in rec["imports"].items():
            mod = importlib.import_module(package)
            for name in names:
                assert name == "*" or callable(getattr(mod, name)), (module, package, name)
        for qualified, call in rec["calls"].items():
            package, name = qualified.rsplit(".", 1)
            fn = getattr(importlib.import_module(package), name)
            params = list(inspect.signature(fn).parameters)
            assert set(call["keywords"]) <= set(params), (module, qualified, params)
            assert call["positional"] <= len(params), (module, qualified)
            seen.add(qualified)
    assert {"torch_scatter.segment_csr", "torch_scatter.gather_csr", "torch_scatter.scatter_mean", "torch_scatter.scatter_std",
            "torch_geometric.utils.scatter", "torch_geometric.utils.softmax", "torch_geometric.utils.cumsum"} <= seen
    # the documented parameter order of the packages
    assert list(inspect.signature(torch_scatter.segment_csr).parameters) == ["src", "indptr", "out", "reduce"]
    assert list(inspect.signature(torch_scatter.gather_csr).parameters) == ["src", "indptr", "out"]
    assert list(inspect.signature(torch_scatter.scatter).parameters) == ["src", "index", "dim", "out", "dim_size", "reduce"]
    assert list(inspect.signature(torch_scatter.scatter_std).parameters) == ["src", "index", "dim", "out", "dim_size", "unbiased"]
    assert list(inspect.signature(torch_geometric.utils.scatter).parameters) == ["src", "index", "dim", "dim_size", "reduce"]
    assert list(inspect.signature(torch_geometric.utils.softmax).parameters) == ["src", "index", "ptr", "num_nodes", "dim"]
    assert list(inspect.signature(torch_geometric.utils.cumsum).parameters) == ["x", "dim"]


def test_cpu_tensors_and_unsupported_layouts_are_refused():
    import torch_scatter
    from torch_geometric.utils import cumsum, scatter, softmax

    x, ptr, index = torch.zeros(4, 3), torch.tensor([0, 2, 4]), torch.tensor([0, 0, 1, 1])
    for call in (lambda: torch_scatter.segment_csr(x, ptr), lambda: torch_scatter.segment_max_csr(x, ptr),
                 lambda: torch_scatter.gather_csr(x[:2], ptr), lambda: torch_scatter.scatter(x, index),
                 lambda: torch_scatter.scatter_mean(x, index, dim=0), lambda: torch_scatter.scatter_std(x, index),
                 lambda: scatter(x, index, reduce="sum"), lambda: softmax(x, ptr=ptr), lambda: softmax(x, index), lambda: cumsum(ptr)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(NotImplementedError):
        torch_scatter.segment_csr(x, ptr.view(1, 3).expand(4, 3))      # a batched indptr
    with pytest.raises(NotImplementedError):
        torch_scatter.gather_csr(x, ptr.view(1, 3))
    with pytest.raises(NotImplementedError):
        softmax(x, ptr=ptr.view(1, 3).expand(4, 3))
    for dim in (1, -1):
        with pytest.raises(NotImplementedError):
            torch_scatter.scatter(x, index, dim=dim)
        with pytest.raises(NotImplementedError):
            softmax(x, ptr=ptr, dim=dim)
    with pytest.raises(ValueError):
        torch_scatter.segment_csr(x, ptr, reduce="mul")


def test_workspace_size_is_monotone_and_aligned():
    from generativedensification_amd import _lib as L
    from generativedensification_amd import segment

    lib = L.load()
    assert segment.ROWS == L.GDR_SEG_ROWS
    r = segment.ROWS
    for c in (1, 3, 160, 264):
        prev = 0
        for n in (0, 1, r - 1, r, r + 1, 4 * r + 64, 12_000, 96_000):
            b = lib.gdr_seg_reduce_bytes(n, 5, c)
            assert b >= prev and b % 256 == 0 and b > 0
            prev = b
        assert lib.gdr_seg_reduce_bytes(96_000, 5, c) >= 2 * (96_000 // r) * c * 12
    assert lib.gdr_seg_reduce_bytes(1000, 7, 8) <= lib.gdr_seg_reduce_bytes(1000, 7, 9) <= lib.gdr_seg_reduce_bytes(1000, 9, 9)
    assert lib.gdr_seg_reduce_bytes(-1, 1, 1) == 0 and b"seg" in lib.gdr_last_error()
    assert lib.gdr_seg_reduce_bytes(10, 1, 0) == 0
    # argument errors are reported before any device work
    assert lib.gdr_seg_reduce(None, 4, None, None, 10, 2, 4, 2, 0, None, 0, None, None, None) == -1
    assert lib.gdr_seg_reduce(0x1000, 4, None, 0x1000, 10, 2, 4, 3, 1, 0x1000, 1 << 20, 0x1000, None, None) == -1   # int64 mean
    assert b"int64" in lib.gdr_last_error()
    assert lib.gdr_seg_reduce(0x1000, 4, None, 0x1000, 10, 2, 4, 2, 0, 0x1000, 16, 0x1000, None, None) == L.GDR_ERR_WORKSPACE
    assert lib.gdr_seg_gather(0x1000, 4, 0x1000, None, 10, 2, 4, 3, 1, 0, 0x1000, None) == -1
    assert lib.gdr_seg_route(0x1000, 0x1000, 10, 2, 4, 3, 0x1000, None) == -1
    assert lib.gdr_seg_ptr_from_sorted(None, None, 10, 2, 0x1000, None) == -1
