"""CPU: the restatement of the densification masks (tests/densify_ref.py) against torch on the CPU — the count formula against
the reference's expression, the masks against a sort-and-rank evaluation written here from torch operators, the gate and split
gradients against autograd in float64; the recorded surface (tests/golden/densify_surface.json) against what densify.py exports;
the refusals that need no GPU."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import densify_cases as DC
import densify_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def densify():
    from generativedensification_amd import densify as D

    return D


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_k_of_equals_the_torch_expression_for_every_n(dtype):
    n = torch.arange(0, 70_001, dtype=torch.long)
    finite = torch.isfinite(n.to(TORCH_DT[dtype]))
    assert finite.sum() >= 65_504
    for ratio in (0.3, 1.0 / 3.0, 0.5, 0.8, 0.9, 0.999):
        want = (float(ratio) * n.to(TORCH_DT[dtype])).ceil().double().numpy()
        got = R.k_of(n.numpy(), ratio, dtype)
        assert np.array_equal(got[finite.numpy()], want[finite.numpy()]), (dtype, ratio)
        assert np.isinf(got[~finite.numpy()]).all()
    assert R.k_of(12000, 0.9, "bf16") == 10816 and R.k_of(12000, 0.9, "f32") == 10800
    assert R.k_of(259, 0.999, "bf16") > 259                 # the clamp: the whole segment


def torch_rank_in_segment(x, sizes):
    """rank of every row inside its segment by descending value: a global descending sort, then a stable sort by segment"""
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    _, perm = torch.sort(x, descending=True)
    _, bperm = torch.sort(batch[perm], stable=True)
    rows = perm[bperm]                                       # rows in ranked order, segment after segment
    starts = torch.cumsum(torch.tensor([0] + sizes[:-1]), 0)
    rank = torch.empty(x.numel(), dtype=torch.long)
    rank[rows] = torch.arange(x.numel()) - starts[batch]
    return rows, rank, batch


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("sizes", [[1], [2, 1, 0, 3], [300, 255, 7], [0, 260, 0, 31]], ids=str)
def test_masks_equal_a_torch_evaluation_on_distinct_values(sizes, dtype):
    n = sum(sizes)
    offset = np.cumsum(sizes)
    for ratio in DC.RATIOS + (0.999,):
        # top-k: distinct values of any sign
        x = torch.from_numpy(DC.distinct_in(dtype, n, seed=n)).to(TORCH_DT[dtype])
        assert torch.unique(x).numel() == n
        _, rank, batch = torch_rank_in_segment(x.float(), sizes)
        k = (float(ratio) * torch.tensor(sizes).to(x.dtype)).ceil().to(torch.long)
        want = rank < k[batch]
        mask, new_offset = R.top_k(x.double().numpy(), ratio, offset, dtype)
        assert np.array_equal(mask, want.numpy()), (ratio, "top_k")
        assert np.array_equal(new_offset, torch.cumsum(torch.minimum(k, torch.tensor(sizes)), 0).numpy())
        # top-p: distinct non-negative values with segment totals around the ratio; the prefix sum as a lower-triangular matmul
        # in float32, cast to the dtype and compared with the Python scalar
        p = torch.from_numpy(DC.distinct_in(dtype, n, seed=n + 1, positive=True)).to(TORCH_DT[dtype]).float()
        batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
        total = torch.zeros(len(sizes)).index_add_(0, batch, p)
        scale = torch.exp2(torch.floor(torch.log2(1.3 / torch.where(total > 0, total, torch.ones(())))))    # (exact: stays distinct)
        p = (p * scale[batch]).to(TORCH_DT[dtype])
        assert all(torch.unique(p[batch == b]).numel() == s for b, s in enumerate(sizes))     # distinct inside every segment
        rows, _, _ = torch_rank_in_segment(p.float(), sizes)
        cums, a = [], 0
        for s in sizes:
            cums.append(torch.tril(torch.ones(s, s)) @ p[rows[a:a + s]].float())
            a += s
        selected = torch.cat(cums).to(p.dtype) <= ratio
        want = torch.zeros(n, dtype=torch.bool)
        want[rows[selected]] = True
        # rows whose float32 triangular sum and float64 running sum round apart may differ: none do when the two masks agree with
        # the restatement's band of one float32 rounding per addition
        lo, hi = R.top_p_band(p.double().numpy(), ratio, offset, dtype, delta=max(sizes) * 2.0 ** -24)
        decided = lo == hi
        assert np.array_equal(want.numpy()[decided], lo[decided]), (ratio, "top_p")
        assert (~decided).sum() <= 2 * len(sizes)
        exact, new_offset = R.top_p(p.double().numpy(), ratio, offset, dtype)
        assert np.array_equal(new_offset, np.cumsum([exact[a:e].sum() for a, e in R.segments(offset, n)]))


def test_ranking_rule():
    x = np.array([0.5, np.nan, -0.0, 0.0, 0.5, -1.0, np.inf, np.nan])
    assert R.ranking(x).tolist() == [1, 7, 6, 0, 4, 2, 3, 5]
    mask, new_offset = R.top_k(x, 0.5, [8], "f32")
    assert mask.tolist() == [True, True, False, False, False, False, True, True] and new_offset.tolist() == [4]
    # offsets are clamped to [previous end, N]; rows behind the last end are never selected
    assert R.clamped_ends([3, 2, 99, 5], 6).tolist() == [3, 3, 6, 6]
    mask, new_offset = R.top_k(np.arange(6.0), 0.5, [4], "f32")
    assert mask.tolist() == [False, False, True, True, False, False] and new_offset.tolist() == [2]
    # top-p: a largest value above the ratio selects nothing, a total below it everything
    mask, new_offset = R.top_p(np.array([0.9, 0.05, 0.1, 0.2, 0.3]), 0.8, [2, 5], "f32")
    assert mask.tolist() == [False, False, True, True, True] and new_offset.tolist() == [0, 3]


@pytest.mark.parametrize("masked", [False, True])
def test_gate_restatement_agrees_with_autograd(masked):
    rng = np.random.default_rng(5)
    n, c = 37, 16
    feat, prob, g = rng.standard_normal((n, c)), rng.random(n), rng.standard_normal((n, c))
    mask = DC.mask_of("random", n) if masked else None
    f_t, p_t = torch.from_numpy(feat).requires_grad_(True), torch.from_numpy(prob).requires_grad_(True)
    hard = f_t * torch.from_numpy(mask)[:, None] if masked else f_t
    out = (hard - f_t * p_t[:, None]).detach() + f_t * p_t[:, None]
    out.backward(torch.from_numpy(g))
    assert np.abs(R.ste_gate(feat, prob, mask) - out.detach().numpy()).max() <= 1e-15
    dfeat, dprob = R.ste_gate_grad(feat, prob, g)
    assert np.abs(dfeat - f_t.grad.numpy()).max() <= 1e-14 and np.abs(dprob - p_t.grad.numpy()).max() <= 1e-13


@pytest.mark.parametrize("gated", [False, True])
def test_split_restatement_agrees_with_autograd(gated):
    rng = np.random.default_rng(6)
    n, c = 41, 8
    feat, prob, coord = rng.standard_normal((n, c)), rng.random(n), rng.standard_normal((n, 3))
    mask = DC.mask_of("random", n)
    m_t = torch.from_numpy(mask)
    f_t, p_t, c_t = (torch.from_numpy(a).requires_grad_(True) for a in (feat, prob, coord))
    gate = (f_t - f_t * p_t[:, None]).detach() + f_t * p_t[:, None] if gated else f_t
    outs = (c_t[m_t], gate[m_t], c_t[~m_t], gate[~m_t])
    grads = [rng.standard_normal(tuple(o.shape)) for o in outs]
    torch.autograd.backward(outs, [torch.from_numpy(g) for g in grads])
    for got, want in zip(R.split_rows(mask, coord, feat), outs):
        assert got.shape == tuple(want.shape) and np.abs(got - want.detach().numpy()).max() <= 1e-15     # ((a - b) + b loses 2u|a|)
    dcoord, dfeat, dprob = R.split_rows_grad(mask, feat, prob if gated else None, *grads)
    assert np.abs(dcoord - c_t.grad.numpy()).max() == 0 and np.abs(dfeat - f_t.grad.numpy()).max() <= 1e-14
    if gated:
        assert np.abs(dprob - p_t.grad.numpy()).max() <= 1e-13
    else:
        assert dprob is None and p_t.grad is None


def test_surface_matches_the_reference():
    surface = json.load(open(os.path.join(HERE, "golden", "densify_surface.json")))
    D = densify()
    for name in ("top_k", "top_p"):
        assert list(inspect.signature(getattr(D, name)).parameters) == surface[name]["params"]
    assert surface["top_k"]["params"] == ["x", "ratio", "batch"] and surface["top_p"]["params"] == ["x", "ratio", "offset"]
    for cls, fn in (("MaskModule", D.mask_module_forward), ("MaskResModule", D.mask_res_module_forward)):
        assert list(inspect.signature(fn).parameters) == surface[cls]["forward"]
        src = inspect.getsource(fn) + inspect.getsource(D._non_leaf)
        used = {a for a in surface[cls]["attributes"] if f"self.{a}" in src}
        assert used <= set(surface[cls]["attributes"]) and {"net", "non_leaf_ratio", "mask_sampling_type"} <= used
        assert surface[cls]["sampling_types"] == ["topk", "topp"]
    assert list(D.POINT_KEYS) == surface["MaskModule"]["point_keys"]
    assert list(D.LEAF_POINT_KEYS) == surface["MaskModule"]["leaf_point_keys"]
    assert list(D.MASK_RES_KEYS) == surface["MaskResModule"]["update_keys"]
    assert "temperature" in surface["MaskResModule"]["attributes"]
    for name in ("segment_top_k", "segment_top_p"):
        assert list(inspect.signature(getattr(D, name)).parameters) == ["x", "ratio", "offset"]
    assert list(inspect.signature(D.ste_gate).parameters) == ["feat", "prob", "mask"]
    assert list(inspect.signature(D.split_rows).parameters) == ["mask", "coord", "feat", "prob", "n_selected"]


def test_refusals_that_need_no_gpu():
    D = densify()
    x, offset = torch.rand(6), torch.tensor([6])
    feat, prob, mask, coord = torch.zeros(6, 16), torch.rand(6, 1), torch.ones(6, dtype=torch.bool), torch.zeros(6, 3)
    for call in (lambda: D.segment_top_k(x, 0.5, offset), lambda: D.segment_top_p(x, 0.5, offset), lambda: D.top_p(x, 0.5, offset),
                 lambda: D.top_k(x, 0.5, torch.zeros(6, dtype=torch.long)), lambda: D.ste_gate(feat, prob),
                 lambda: D.ste_gate(feat, prob, mask), lambda: D.split_rows(mask, coord, feat, prob)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
        D.segment_top_k(x.double(), 0.5, offset)
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
        D.ste_gate(feat.double(), prob)
    with pytest.raises(TypeError, match="integer tensor"):
        D.segment_top_p(x, 0.5, offset.float())
    with pytest.raises(TypeError, match="bool tensor"):
        D.split_rows(mask.long(), coord, feat)
    with pytest.raises(TypeError, match="must be a tensor"):
        D.segment_top_k(x, 0.5, [6])
    for ratio in (0.0, 1.0, -0.1, 1.5, float("nan"), 1.0 - 2.0 ** -30):
        with pytest.raises(ValueError, match="ratio must lie"):
            D.segment_top_k(x, ratio, offset)
        with pytest.raises(ValueError, match="ratio must lie"):
            D.top_p(x, ratio, offset)
    with pytest.raises(ValueError, match="segments are outside"):
        D.segment_top_k(x, 0.5, torch.zeros(0, dtype=torch.long))
    with pytest.raises(ValueError, match="segments are outside"):
        D.segment_top_p(x, 0.5, torch.zeros(1025, dtype=torch.long))
    with pytest.raises(ValueError, match="must be \\(N,\\) or \\(N, 1\\)"):
        D.segment_top_k(torch.rand(6, 2), 0.5, offset)
    for c in (12, 1032):
        with pytest.raises(ValueError, match="multiple of 8"):
            D.ste_gate(torch.zeros(6, c), prob)
        with pytest.raises(ValueError, match="multiple of 8"):
            D.split_rows(mask, coord, torch.zeros(6, c))
    with pytest.raises(ValueError, match="n_selected"):
        D.split_rows(mask, coord, feat, prob, n_selected=7)
    # the C entry points refuse the same before any launch
    lib = __import__("generativedensification_amd._lib", fromlist=["load"]).load()
    fake, f32 = 0x1000, 2                            # never dereferenced: every refusal happens before a launch
    assert lib.gdr_densify_select(fake, f32, fake, 8, 0, 0, 0.5, 0.5, fake, 1 << 20, fake, fake, None) == -1         # B = 0
    assert lib.gdr_densify_select(fake, f32, fake, 8, 1025, 0, 0.5, 0.5, fake, 1 << 20, fake, fake, None) == -3      # B > 1024
    assert lib.gdr_densify_select(fake, f32, fake, (1 << 30) + 1, 1, 0, 0.5, 0.5, fake, 1 << 20, fake, fake, None) == -3
    assert lib.gdr_densify_select(fake, 7, fake, 8, 1, 0, 0.5, 0.5, fake, 1 << 20, fake, fake, None) == -1           # dtype
    assert lib.gdr_densify_select(fake, f32, fake, 8, 1, 2, 0.5, 0.5, fake, 1 << 20, fake, fake, None) == -1         # mode
    assert lib.gdr_densify_select(fake, f32, fake, 8, 1, 0, 1.0, 0.5, fake, 1 << 20, fake, fake, None) == -1         # ratio
    assert b"ratio" in lib.gdr_last_error()
    assert lib.gdr_densify_select(fake, f32, fake, 8, 1, 0, 0.5, 0.5, fake, 16, fake, fake, None) == -4              # workspace
    assert lib.gdr_densify_select(fake, f32, fake + 4, 8, 1, 0, 0.5, 0.5, fake, 1 << 20, fake, fake, None) == -1     # unaligned
    assert lib.gdr_densify_gate_forward(fake, 12, f32, None, 4, 12, fake, f32, None) == -3                           # C % 8
    assert b"multiple of 8" in lib.gdr_last_error()
    assert lib.gdr_densify_gate_forward(fake, 16, f32, None, 0, 16, fake, f32, None) == 0                            # N = 0
    assert lib.gdr_densify_gate_forward(fake + 4, 16, f32, None, 4, 16, fake, f32, None) == -1                       # unaligned
    assert lib.gdr_densify_split_scan(fake, 4, fake, 16, fake, fake, None) == -4                                     # workspace
    assert lib.gdr_densify_split_forward(fake, fake, 4, 16, fake, 16, f32, fake, 3, 3, 2, 2, fake, fake, f32, fake, fake, None) == -1
    assert b"coord_elem_bytes" in lib.gdr_last_error()
    assert lib.gdr_densify_rows_backward(fake, fake, 4, 2048, fake, fake, 2048, f32, 2, 2, fake, 2048, f32, None, 0, None, None, 0, 4,
                                         fake, None, None, None) == -3                                               # C > 1024
    for bad in ((-1, 1), (4, 0), (4, 1025), ((1 << 30) + 1, 1)):
        assert lib.gdr_densify_select_bytes(*bad) == 0
    prev = 0
    for n in (0, 1, 1023, 1024, 1025, 36_000, 1 << 20, 1 << 30):
        nbytes = lib.gdr_densify_select_bytes(n, 3)
        assert nbytes >= prev and nbytes > 0 and nbytes % 256 == 0 and nbytes >= 24 * n
        prev = nbytes
        assert lib.gdr_densify_split_bytes(n) > 0 and lib.gdr_densify_split_bytes(n) % 256 == 0
