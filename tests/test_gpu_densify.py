"""GPU: the densification masks (csrc/densify.hip through generativedensification_amd.densify) against the float64 / integer
restatement (tests/densify_ref.py).

Selection is compared bit for bit: top-k everywhere, top-p where every float32 sum is exact (dyadic values).  top-p on general
values is compared on the rows the restatement decides (see test_top_p_accuracy).  Gate and split run on small integers, where
every product and sum is exact, and are compared bit for bit too."""
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import densify_cases as DC
import densify_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TD = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
NAME = {v: k for k, v in TD.items()}


def densify():
    from generativedensification_amd import densify as D

    return D


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(TD[dtype]) if dtype is not None else t).to(DEV)


def f64(t):
    return t.detach().double().cpu().numpy()


def twice(fn, *args):
    """the call's results, after checking that a second call gives the same bits"""
    a, b = fn(*args), fn(*args)
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and torch.equal(u, v), "two calls differ"
    return a


def check_selection(got, want, what):
    mask, new_offset = got
    assert mask.dtype == torch.bool and new_offset.dtype == torch.int64 and mask.dim() == 1, what
    bad = np.flatnonzero(mask.cpu().numpy() != want[0])
    assert bad.size == 0, (what, bad[:8], bad.size)
    assert np.array_equal(new_offset.cpu().numpy(), want[1]), (what, new_offset.cpu().numpy(), want[1])


# ---- selection, bit-exact -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("layout", list(DC.LAYOUTS))
def test_top_k_equals_the_restatement(layout, dtype):
    D = densify()
    offset, n = DC.offsets(layout)
    off = dev(offset)
    for seed, kind in enumerate(("distinct", "five", "sigmoid", "special")):
        x = dev(DC.values(kind, n, seed + n), dtype)
        x64 = f64(x)
        for ratio in DC.RATIOS:
            check_selection(twice(D.segment_top_k, x, ratio, off), R.top_k(x64, ratio, offset, dtype), (layout, dtype, kind, ratio))
    # (N, 1) scores and an int32 offset are taken as they are
    x = dev(DC.values("five", n, 1), dtype)
    check_selection(D.segment_top_k(x[:, None], 0.5, off.int()), R.top_k(f64(x), 0.5, offset, dtype), (layout, dtype, "column"))


def test_top_k_bf16_sigmoid_scores_have_heavy_ties_and_a_defined_outcome():
    D = densify()
    offset, n = DC.offsets("three_samples")
    x = dev(DC.values("sigmoid", n, 11), "bf16")
    assert torch.unique(x).numel() < 1000                     # a few hundred distinct values over 36 000 points
    mask, new_offset = twice(D.segment_top_k, x, 0.9, dev(offset))
    assert new_offset.tolist() == [10816, 2 * 10816, 3 * 10816]                       # not 10 800: the count is rounded to bf16
    x64 = f64(x)
    for a, e in R.segments(offset, n):                        # the tie rule, stated with numpy's stable sort
        want = np.zeros(e - a, dtype=bool)
        want[np.argsort(-x64[a:e], kind="stable")[:10816]] = True
        assert np.array_equal(mask[a:e].cpu().numpy(), want)


def test_top_k_selects_the_whole_segment_where_k_exceeds_n():
    D = densify()
    x = dev(DC.values("distinct", 259 + 300, 3), "bf16")
    offset = np.array([259, 559])
    assert R.k_of(259, 0.999, "bf16") > 259 and R.k_of(300, 0.999, "bf16") == 300
    mask, new_offset = twice(D.segment_top_k, x, 0.999, dev(offset))
    assert mask.all() and new_offset.tolist() == [259, 559]
    check_selection((mask, new_offset), R.top_k(f64(x), 0.999, offset, "bf16"), "clamp")
    # f16: a segment whose length is not finite in the dtype is selected whole
    n = 66_000
    x = dev(DC.values("five", n, 4), "f16")
    mask, new_offset = D.segment_top_k(x, 0.5, dev(np.array([n])))
    assert mask.all() and new_offset.tolist() == [n]


def test_offsets_are_clamped_on_the_device():
    D = densify()
    x = dev(DC.values("distinct", 40, 5), "f32")
    for offset in ([10, 5, 99, 20], [-3, 40], [50], [0, 0, 0]):
        off = np.asarray(offset, dtype=np.int64)
        check_selection(twice(D.segment_top_k, x, 0.5, dev(off)), R.top_k(f64(x), 0.5, off, "f32"), offset)
        check_selection(twice(D.segment_top_p, x.abs() / 64, 0.5, dev(off)), R.top_p(f64(x.abs() / 64), 0.5, off, "f32"), offset)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("layout", list(DC.LAYOUTS))
def test_top_p_equals_the_restatement_where_the_sums_are_exact(layout, dtype):
    D = densify()
    offset, n = DC.offsets(layout)
    off = dev(offset)
    for scale in (1.0, 64.0):                                 # totals of a 12 000-row segment: 1.4 and 88; of a 256-row one: 0.03 and 1.9
        x = dev(DC.values("dyadic", n, n) * scale, dtype)
        x64 = f64(x)
        assert np.array_equal(x64, DC.values("dyadic", n, n) * scale)
        for ratio in DC.RATIOS:
            check_selection(twice(D.segment_top_p, x, ratio, off), R.top_p(x64, ratio, offset, dtype), (layout, dtype, scale, ratio))
    check_selection(D.top_p(x[:, None], 0.5, off), R.top_p(x64, 0.5, offset, dtype), (layout, dtype, "reference signature"))


def test_reference_signature_top_k_takes_the_batch_vector():
    D = densify()
    offset, n = DC.offsets("empty_middle")
    sizes = DC.LAYOUTS["empty_middle"][0]
    batch = dev(np.repeat(np.arange(len(sizes)), sizes))
    x = dev(DC.values("distinct", n, 2), "f32")
    check_selection(D.top_k(x[:, None], 0.5, batch), R.top_k(f64(x), 0.5, offset, "f32"), "top_k(batch)")
    mask, new_offset = D.top_k(x[:0], 0.5, batch[:0])
    assert mask.shape == (0,) and new_offset.shape == (0,)


# ---- top-p accuracy -------------------------------------------------------------------------------------------------------

DELTA = 2.0 ** -18


def top_p_inputs(case):
    rng = np.random.default_rng(7)
    if case == "nothing_everything_and_a_cut":
        sizes = [50, 40, 3000]
        x = np.concatenate([np.r_[0.9, rng.random(49) * 0.01], rng.random(40) * 0.5 / 40, rng.random(3000) / 1500])
    else:
        sizes = [12000]
        x = rng.random(12000)
        x = x / x.sum()
    return np.cumsum(sizes), x


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", ["nothing_everything_and_a_cut", "uniform_12000"])
def test_top_p_accuracy(case, dtype):
    """Prefix sums in float64 on the inputs as rounded to their dtype.  A row is decided if the comparison gives the same answer
    for prefix (1 - delta) and prefix (1 + delta), delta = 2^-18: no path of the kernel's scan tree holds more than 34 float32
    additions (3 inside a thread, 8 across the workgroup, 1 to join them, 10 + 10 across the two carry levels, 2 to join the
    carry), each with unit roundoff 2^-24, which 64 * 2^-24 covers.  Decided rows must match; at most 4 rows per segment are
    undecided (asserted on the restatement alone)."""
    D = densify()
    offset, x64 = top_p_inputs(case)
    x = dev(x64, dtype)
    x64 = f64(x)
    for ratio in DC.RATIOS:
        lo, hi = R.top_p_band(x64, ratio, offset, dtype, DELTA)
        decided = lo == hi
        for a, e in R.segments(offset, x64.size):
            assert (~decided[a:e]).sum() <= 4, (case, dtype, ratio)
        mask, new_offset = twice(D.segment_top_p, x, ratio, dev(offset))
        got = mask.cpu().numpy()
        print(f"top-p {case}/{dtype}/{ratio:.3f}: undecided={int((~decided).sum())} selected={int(got.sum())} "
              f"band=[{int(lo.sum())}, {int(hi.sum())}]")
        assert np.array_equal(got[decided], lo[decided]), (case, dtype, ratio)
        assert np.array_equal(new_offset.cpu().numpy(), R.counts_to_offset(got, offset))
        if case == "nothing_everything_and_a_cut":
            assert not got[:50].any() and got[50:90].all() and 0 < got[90:].sum() < 3000


# ---- gate and split -------------------------------------------------------------------------------------------------------

MIXES = [("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32")]


def same(got, want64, dtype, what):
    want = torch.from_numpy(np.ascontiguousarray(want64)).to(dtype)
    assert got.dtype == dtype and got.shape == want.shape and torch.equal(got.cpu(), want), what


@pytest.mark.parametrize("mix", MIXES, ids="-".join)
@pytest.mark.parametrize("shape", DC.GATE_SHAPES, ids=str)
def test_ste_gate_on_integers(shape, mix):
    D = densify()
    n, c = shape
    feat64, prob64, g64 = DC.integers((n, c), 1), DC.integers((n, 1), 2, 0, 4), DC.integers((n, c), 3, -4, 4)
    res = torch.promote_types(TD[mix[0]], TD[mix[1]])
    for kind in (None,) + DC.MASKS:
        mask = None if kind is None else DC.mask_of(kind, n)
        feat, prob = dev(feat64, mix[0]).requires_grad_(True), dev(prob64, mix[1]).requires_grad_(True)
        out = D.ste_gate(feat, prob, None if mask is None else dev(mask))
        out.backward(dev(g64).to(res))
        same(out.detach(), R.ste_gate(feat64, prob64, mask), res, (shape, mix, kind, "out"))
        dfeat, dprob = R.ste_gate_grad(feat64, prob64, g64)
        same(feat.grad, dfeat, TD[mix[0]], (shape, mix, kind, "dfeat"))
        same(prob.grad, dprob[:, None], TD[mix[1]], (shape, mix, kind, "dprob"))


@pytest.mark.parametrize("mix", MIXES, ids="-".join)
@pytest.mark.parametrize("shape", DC.GATE_SHAPES, ids=str)
def test_split_rows_on_integers(shape, mix):
    D = densify()
    n, c = shape
    feat64, prob64, coord64 = DC.integers((n, c), 4), DC.integers((n,), 5, 0, 4), DC.integers((n, 3), 6, -100, 100)
    res = torch.promote_types(TD[mix[0]], TD[mix[1]])
    for kind in DC.MASKS + ("random",):
        mask = DC.mask_of(kind, n)
        for gated in (True, False):
            feat, coord = dev(feat64, mix[0]).requires_grad_(True), dev(coord64, "f32").requires_grad_(True)
            prob = dev(prob64, mix[1]).requires_grad_(True) if gated else None
            out_dt = res if gated else TD[mix[0]]
            outs = D.split_rows(dev(mask), coord, feat, prob)
            wants = R.split_rows(mask, coord64, feat64)
            for o, w, dt in zip(outs, wants, (torch.float32, out_dt, torch.float32, out_dt)):
                same(o.detach(), w, dt, (shape, mix, kind, gated, "forward"))           # (row order kept)
            grads64 = [DC.integers(tuple(o.shape), 7 + i, -4, 4) for i, o in enumerate(outs)]
            torch.autograd.backward(outs, [dev(g).to(o.dtype) for g, o in zip(grads64, outs)])
            dcoord, dfeat, dprob = R.split_rows_grad(mask, feat64, prob64 if gated else None, *grads64)
            same(coord.grad, dcoord, torch.float32, (shape, mix, kind, gated, "dcoord"))
            same(feat.grad, dfeat, TD[mix[0]], (shape, mix, kind, gated, "dfeat"))
            if gated:
                same(prob.grad, dprob, TD[mix[1]], (shape, mix, kind, gated, "dprob"))
            # the count given: the same bits
            again = D.split_rows(dev(mask), coord.detach(), feat.detach(), None if prob is None else prob.detach(), int(mask.sum()))
            assert all(torch.equal(a, o.detach()) for a, o in zip(again, outs))


def test_integer_coordinates_and_strided_inputs():
    D = densify()
    n, c = 257, 160
    mask = DC.mask_of("random", n)
    for dtype in ("f32", "bf16"):
        wide = dev(DC.integers((n, c + 16), 8), dtype)
        feat = wide[:, 8:8 + c]                                 # a column slice: row stride c + 16, not contiguous
        probs = dev(DC.integers((n, 2), 9, 0, 4), dtype)
        prob = probs[:, 1]
        grid = dev(DC.integers((n, 3), 10, 0, 500).astype(np.int64))
        assert not feat.is_contiguous() and not prob.is_contiguous()
        f, p = feat.detach().requires_grad_(True), prob.detach().requires_grad_(True)     # (detach keeps the strides)
        assert f.stride() == feat.stride()
        outs = D.split_rows(dev(mask), grid, f, p)
        wants = R.split_rows(mask, f64(grid), f64(feat))
        assert outs[0].dtype == torch.int64 and not outs[0].requires_grad
        for o, w in zip(outs, wants):
            assert torch.equal(o.detach().double().cpu(), torch.from_numpy(w).double())
        g_sel, g_rest = DC.integers(tuple(outs[1].shape), 11, -4, 4), DC.integers(tuple(outs[3].shape), 12, -4, 4)
        torch.autograd.backward([outs[1], outs[3]], [dev(g_sel, dtype), dev(g_rest, dtype)])
        _, dfeat, dprob = R.split_rows_grad(mask, f64(feat), f64(prob), np.zeros((len(g_sel), 3)), g_sel, np.zeros((len(g_rest), 3)), g_rest)
        same(f.grad, dfeat, TD[dtype], "strided dfeat")
        same(p.grad, dprob, TD[dtype], "strided dprob")
        gate = D.ste_gate(feat, prob[:, None], dev(mask))
        same(gate, R.ste_gate(f64(feat), None, mask), TD[dtype], "strided gate")


@pytest.mark.parametrize("mix", MIXES, ids="-".join)
def test_ste_gate_forward_against_the_torch_expression(mix):
    """(a - b) + b can lose 2u |a|, u the unit roundoff of the result dtype; ours returns a itself"""
    D = densify()
    rng = np.random.default_rng(13)
    feat, prob = dev(rng.standard_normal((257, 160)), mix[0]), dev(rng.random((257, 1)), mix[1])
    mask = dev(DC.mask_of("random", 257))
    res = torch.promote_types(feat.dtype, prob.dtype)
    u = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8}[res]
    for m in (None, mask):
        hard = feat if m is None else feat * m[:, None]
        want = (hard - feat * prob).detach() + feat * prob
        got = D.ste_gate(feat, prob, m)
        assert got.dtype == want.dtype == res
        assert bool(((got.double() - want.double()).abs() <= 2 * u * feat.double().abs()).all())
        assert torch.equal(got, hard.to(res))


# ---- behaviour ------------------------------------------------------------------------------------------------------------

def test_runs_under_vjp_and_under_no_grad():
    D = densify()
    n, c = 257, 16
    feat, prob, coord = dev(DC.integers((n, c), 1), "f32"), dev(DC.integers((n,), 2, 0, 4), "f32"), dev(DC.integers((n, 3), 3), "f32")
    mask = dev(DC.mask_of("random", n))
    g = dev(DC.integers((n, c), 4), "f32")
    out, (dfeat, dprob) = torch.autograd.functional.vjp(lambda a, b: D.ste_gate(a, b, mask), (feat, prob), g)
    a, b = feat.clone().requires_grad_(True), prob.clone().requires_grad_(True)
    o = D.ste_gate(a, b, mask)
    o.backward(g)
    assert torch.equal(out, o) and torch.equal(dfeat, a.grad) and torch.equal(dprob, b.grad)
    k = int(mask.sum())
    outs, grads = torch.autograd.functional.vjp(lambda co, fe, pr: D.split_rows(mask, co, fe, pr), (coord, feat, prob),
                                                (coord[:k], g[:k], coord[k:], g[k:]))
    co, fe, pr = (t.clone().requires_grad_(True) for t in (coord, feat, prob))
    outs2 = D.split_rows(mask, co, fe, pr)
    torch.autograd.backward(outs2, (coord[:k], g[:k], coord[k:], g[k:]))
    assert all(torch.equal(x, y) for x, y in zip(outs, outs2)) and all(torch.equal(x, y.grad) for x, y in zip(grads, (co, fe, pr)))
    with torch.no_grad():
        assert torch.equal(D.ste_gate(a, b, mask), o) and not D.ste_gate(a, b, mask).requires_grad
        assert all(torch.equal(x, y) and not x.requires_grad for x, y in zip(D.split_rows(mask, co, fe, pr), outs2))
    # only prob wants a gradient
    b2 = prob.clone().requires_grad_(True)
    D.ste_gate(feat, b2, mask).backward(g)
    assert torch.equal(b2.grad, b.grad)
    assert not D.segment_top_k(b, 0.5, dev(np.array([n])))[0].requires_grad       # selection has no gradient


def test_empty_inputs_return_empty_tensors():
    D = densify()
    off = dev(np.array([0, 0]))
    for fn in (D.segment_top_k, D.segment_top_p):
        mask, new_offset = fn(torch.zeros(0, device=DEV), 0.5, off)
        assert mask.shape == (0,) and mask.dtype == torch.bool and new_offset.tolist() == [0, 0]
    feat = torch.zeros(0, 16, device=DEV, requires_grad=True)
    out = D.ste_gate(feat, torch.zeros(0, 1, device=DEV))
    assert out.shape == (0, 16)
    out.sum().backward()
    outs = D.split_rows(torch.zeros(0, dtype=torch.bool, device=DEV), torch.zeros(0, 3, device=DEV), feat)
    assert [tuple(o.shape) for o in outs] == [(0, 3), (0, 16), (0, 3), (0, 16)]


def test_no_host_synchronisation():
    D = densify()
    offset, n = DC.offsets("around_tile")
    off = dev(offset)
    x = dev(DC.values("sigmoid", n, 1), "bf16")
    feat64, coord64 = DC.integers((n, 160), 2), DC.integers((n, 3), 3)
    mask_np = DC.mask_of("random", n)
    mask, k = dev(mask_np), int(mask_np.sum())

    def work():
        feat, prob = dev(feat64, "bf16").requires_grad_(True), dev(f64(x), "f32").requires_grad_(True)
        coord = dev(coord64, "f32")
        torch.cuda.synchronize()
        return feat, prob, coord

    def calls(feat, prob, coord):
        D.segment_top_k(x, 0.8, off)
        D.segment_top_p(x, 0.8, off)
        D.top_p(x, 0.8, off)
        D.ste_gate(feat, prob, mask).sum().backward()
        outs = D.split_rows(mask, coord, feat, prob, n_selected=k)
        (outs[1].sum() + outs[3].sum()).backward()
        return outs

    calls(*work())                                   # warm-up: library load, kernel images
    args = work()
    torch.cuda.synchronize()
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        raised = False
        try:
            off[-1].item()                           # the canary: what a read-back does
        except RuntimeError:
            raised = True
        if raised:
            outs = calls(*args)
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    if not raised:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this torch build")
    torch.cuda.synchronize()
    assert outs[1].shape == (k, 160) and torch.isfinite(args[0].grad.float()).all()


def test_a_wrong_n_selected_truncates_and_never_writes_past_the_capacities():
    D = densify()
    from generativedensification_amd import _lib as L
    n, c = 1500, 16
    mask_np = DC.mask_of("random", n)
    k = int(mask_np.sum())
    feat64, coord64 = DC.integers((n, c), 1), DC.integers((n, 3), 2)
    feat, coord, mask = dev(feat64, "f32"), dev(coord64, "f32"), dev(mask_np)
    want = R.split_rows(mask_np, coord64, feat64)
    outs = D.split_rows(mask, coord, feat, None, n_selected=k - 3)
    assert [o.shape[0] for o in outs] == [k - 3, k - 3, n - k + 3, n - k + 3]
    assert np.array_equal(f64(outs[0]), want[0][:k - 3]) and np.array_equal(f64(outs[1]), want[1][:k - 3])
    assert np.array_equal(f64(outs[2])[:n - k], want[2]) and np.array_equal(f64(outs[3])[:n - k], want[3])
    # the entry point itself, with both capacities 3 rows short and sentinel rows behind them
    lib = L.load()
    dest, count = torch.empty(n, dtype=torch.int64, device=DEV), torch.empty(1, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.gdr_densify_split_bytes(n) + 256, dtype=torch.uint8, device=DEV)
    base = (ws.data_ptr() + 255) & ~255
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.gdr_densify_split_scan(mask.data_ptr(), n, base, ws.numel() - 256, dest.data_ptr(), count.data_ptr(), st) == 0
    assert int(count) == k
    guard = 8
    bufs = [torch.full((rows + guard, width), -77.0, device=DEV) for rows, width in ((k - 3, 3), (k - 3, c), (n - k - 3, 3), (n - k - 3, c))]
    assert lib.gdr_densify_split_forward(mask.data_ptr(), dest.data_ptr(), n, c, feat.data_ptr(), c, 2, coord.data_ptr(), 3, 4, k - 3,
                                         n - k - 3, bufs[1].data_ptr(), bufs[3].data_ptr(), 2, bufs[0].data_ptr(), bufs[2].data_ptr(),
                                         st) == 0
    torch.cuda.synchronize()
    for buf, w in zip(bufs, want):
        rows = buf.shape[0] - guard
        assert np.array_equal(f64(buf[:rows]), w[:rows]) and bool((buf[rows:] == -77.0).all())


def test_refusals_on_the_device():
    D = densify()
    x, off = torch.rand(8, device=DEV), dev(np.array([8]))
    feat, prob, mask, coord = (torch.zeros(8, 16, device=DEV), torch.rand(8, device=DEV), torch.ones(8, dtype=torch.bool, device=DEV),
                               torch.zeros(8, 3, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.segment_top_k(x, 0.5, off.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.split_rows(mask, coord.cpu(), feat, prob)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.ste_gate(feat, prob.cpu())
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
        D.segment_top_p(x.double(), 0.5, off)
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
        D.split_rows(mask, coord, feat.double())
    with pytest.raises(ValueError, match="multiple of 8"):
        D.ste_gate(torch.zeros(8, 12, device=DEV), prob)
    with pytest.raises(ValueError, match="multiple of 8"):
        D.split_rows(mask, coord, torch.zeros(8, 12, device=DEV))
    for ratio in (0.0, 1.0, 1.5):
        with pytest.raises(ValueError, match="ratio must lie"):
            D.segment_top_k(x, ratio, off)
        with pytest.raises(ValueError, match="ratio must lie"):
            D.segment_top_p(x, ratio, off)
    for b in (0, 1025):
        with pytest.raises(ValueError, match="segments are outside"):
            D.segment_top_k(x, 0.5, torch.zeros(b, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="segments are outside"):
        D.top_k(x, 0.5, torch.full((8,), 1024, device=DEV))
    with pytest.raises(ValueError, match="prob must have"):
        D.ste_gate(feat, prob[:7])


# ---- the bound modules ----------------------------------------------------------------------------------------------------

class Point(dict):
    """a minimal stand-in for the reference's Point: a dict with attribute access"""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def ranks(score, sizes):
    """rank of every row inside its segment by descending score (torch operators, any device)"""
    batch = torch.repeat_interleave(torch.arange(len(sizes), device=score.device), torch.tensor(sizes, device=score.device))
    _, perm = torch.sort(score.reshape(-1), descending=True)
    _, bperm = torch.sort(batch[perm], stable=True)
    rows = perm[bperm]
    starts = torch.cumsum(torch.tensor([0] + sizes[:-1], device=score.device), 0)
    rank = torch.empty_like(rows)
    rank[rows] = torch.arange(rows.numel(), device=score.device) - starts[batch]
    return rank, batch


def torch_mask_module(net, point, sizes, ratio, mask=None):
    feat = point.feat
    prob = torch.sigmoid(net(feat))
    if mask is None:
        rank, batch = ranks(prob.detach(), sizes)
        k = (float(ratio) * torch.tensor(sizes, device=feat.device).to(prob.dtype)).ceil().long()
        mask = rank < k[batch]
    counts = torch.stack([m.sum() for m in torch.split(mask, sizes)])
    gate = (feat - feat * prob).detach() + feat * prob
    return Point(coord=point.coord[mask], feat=gate[mask], global_feat=point.global_feat, offset=torch.cumsum(counts, 0),
                 grid_size=point.grid_size,
                 leaf_point=Point(coord=point.coord[~mask], feat=gate[~mask], offset=point.offset - torch.cumsum(counts, 0),
                                  grid_size=point.grid_size)), mask


def torch_mask_res_module(net, temperature, point, sizes, ratio, mask=None):
    """The reference's forward keeps its pyg_softmax call, which in this repository is the drop-in of segment.py: the float32
    restatement calls it too, so that the comparison with the bound forward measures the selection and the gate and not two
    softmax backwards against each other (the gradient of the last bias is 0 in exact arithmetic, softmax being
    shift-invariant, so there the errors are cancellation noise of the softmax backward alone).  The float64 run, which the
    drop-in does not serve, takes torch.softmax per segment."""
    feat = point.feat
    raw_prob = net(feat)
    if raw_prob.dtype == torch.float64:
        prob = torch.cat([torch.softmax(z, 0) for z in torch.split(raw_prob / temperature, sizes)])
    else:
        from generativedensification_amd.segment import softmax as pyg_softmax
        prob = pyg_softmax(src=raw_prob.to(torch.float32) / temperature, ptr=F.pad(point.offset, (1, 0), "constant", 0), dim=0)
    if mask is None:
        rank, batch = ranks(prob.detach(), sizes)
        k = (float(ratio) * torch.tensor(sizes, device=feat.device).to(prob.dtype)).ceil().long()
        mask = rank < k[batch]
    counts = torch.cumsum(torch.stack([m.sum() for m in torch.split(mask, sizes)]), 0)
    out = Point(point)
    out.feat = (feat * mask[:, None] - feat * prob).detach() + feat * prob
    out.update({"raw_prob": raw_prob, "prob": prob, "non_leaf": mask, "non_leaf_offset": counts, "leaf": ~mask,
                "leaf_offset": point.offset - counts})
    return out, mask


def assert_cut_is_untied(score, sizes, ratio):
    """the scores on the two sides of every segment's cut differ, so the tie rule cannot change the mask"""
    for z, n in zip(torch.split(score.detach().reshape(-1), sizes), sizes):
        k = int(R.k_of(n, ratio, NAME[score.dtype]))
        ranked = torch.sort(z, descending=True)[0]
        assert k >= n or bool(ranked[k - 1] > ranked[k]), (n, k)


def module_inputs(c, sizes, dtype=torch.float32):
    n = sum(sizes)
    gen = torch.Generator().manual_seed(17)
    net = torch.nn.Sequential(torch.nn.Linear(c, c), torch.nn.GELU(), torch.nn.Linear(c, 1))
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.2)
    point = Point(coord=torch.randn(n, 3, generator=gen), feat=torch.randn(n, c, generator=gen), global_feat=torch.randn(len(sizes), 24, generator=gen),
                  offset=torch.cumsum(torch.tensor(sizes), 0), grid_size=0.01)
    g = torch.randn(n, c, generator=gen)
    return net, point, g


def to_device(net, point, dtype):
    import copy
    net = copy.deepcopy(net).to(DEV, dtype)
    moved = Point({k: (v.to(DEV, dtype) if v.is_floating_point() else v.to(DEV)) if isinstance(v, torch.Tensor) else v
                   for k, v in point.items()})
    return net, moved


def grad_bar(nets, what):
    """e_hip <= 2 e_torch + half an ulp of float32 at max|ref|, per parameter, both against float64"""
    hip, tor, ref = nets
    bad = []
    for (name, ph), pt, pr in zip(hip.named_parameters(), tor.parameters(), ref.parameters()):
        r = pr.grad.double().cpu()
        e_hip, e_torch = float((ph.grad.double().cpu() - r).abs().max()), float((pt.grad.double().cpu() - r).abs().max())
        slack = R_half_ulp(float(r.abs().max()))
        print(f"densify-bar {what}/{name}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} half_ulp={slack:.3e}")
        assert torch.isfinite(ph.grad).all()
        if not e_hip <= 2 * e_torch + slack:
            bad.append((name, e_hip, e_torch, slack))
    assert not bad, bad


def R_half_ulp(magnitude):
    import math
    return 2.0 ** (max(math.floor(math.log2(magnitude)) if magnitude > 0 else -126, -126) - 24)


@pytest.mark.parametrize("sizes", [[700, 1, 1347], [300]], ids=str)
def test_mask_module_forward_bound_onto_a_stand_in(sizes):
    D = densify()
    c, ratio = 160, 0.8
    net, point, g = module_inputs(c, sizes)
    n = sum(sizes)
    runs = {}
    for which, dtype in (("hip", torch.float32), ("torch", torch.float32), ("ref", torch.float64)):
        net_d, point_d = to_device(net, point, dtype)
        if which == "hip":
            module = types.SimpleNamespace(net=net_d, non_leaf_ratio=ratio, temperature=1.0, mask_sampling_type="topk")
            out = D.mask_module_forward(module, point_d)
            mask = torch.zeros(n, dtype=torch.bool, device=DEV)
        else:
            out, mask = torch_mask_module(net_d, point_d, sizes, ratio, None if which == "torch" else runs["torch"][2])
        k = out.feat.shape[0]
        loss = (out.feat * g[:k].to(DEV, dtype)).sum() + (out.leaf_point.feat * g[k:].to(DEV, dtype)).sum() + out.coord.sum()
        loss.backward()
        runs[which] = (out, net_d, mask)
    hip, tor = runs["hip"][0], runs["torch"][0]
    assert type(hip) is Point and list(hip) == list(D.POINT_KEYS) == list(tor) and list(hip.leaf_point) == list(D.LEAF_POINT_KEYS)
    assert_cut_is_untied(torch.sigmoid(runs["torch"][1](to_device(net, point, torch.float32)[1].feat)), sizes, ratio)
    for a, b in ((hip, tor), (hip.leaf_point, tor.leaf_point)):
        for key in ("coord", "feat", "offset"):
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
        assert torch.equal(a.offset, b.offset) and torch.equal(a.coord, b.coord) and a.grid_size == b.grid_size
        assert bool(((a.feat - b.feat).abs() <= 2 * 2.0 ** -24 * a.feat.abs()).all())
    assert hip.global_feat is not None and torch.equal(hip.global_feat, tor.global_feat)
    assert torch.equal(hip.offset + hip.leaf_point.offset, torch.cumsum(torch.tensor(sizes), 0).to(DEV))
    grad_bar([runs[w][1] for w in ("hip", "torch", "ref")], f"MaskModule/{sizes}")
    # ratio 1.0: the branch without a net
    whole = D.mask_module_forward(types.SimpleNamespace(non_leaf_ratio=1.0), to_device(net, point, torch.float32)[1])
    assert list(whole) == list(D.POINT_KEYS) and whole.leaf_point.feat is whole.feat and whole.feat.shape == (n, c)
    # top-p: the same keys, offsets that add up
    module = types.SimpleNamespace(net=runs["hip"][1], non_leaf_ratio=0.5, temperature=1.0, mask_sampling_type="topp")
    out = D.mask_module_forward(module, to_device(net, point, torch.float32)[1])
    assert torch.equal(out.offset + out.leaf_point.offset, torch.cumsum(torch.tensor(sizes), 0).to(DEV))
    assert out.feat.shape[0] == int(out.offset[-1]) and out.leaf_point.feat.shape[0] == n - int(out.offset[-1])


@pytest.mark.parametrize("sizes", [[700, 1, 1347], [300]], ids=str)
def test_mask_res_module_forward_bound_onto_a_stand_in(sizes):
    D = densify()
    c, ratio, temperature = 160, 0.8, 0.7
    net, point, g = module_inputs(c, sizes)
    n = sum(sizes)
    runs = {}
    for which, dtype in (("hip", torch.float32), ("torch", torch.float32), ("ref", torch.float64)):
        net_d, point_d = to_device(net, point, dtype)
        if which == "hip":
            module = types.SimpleNamespace(net=net_d, non_leaf_ratio=ratio, temperature=temperature, mask_sampling_type="topk")
            out = D.mask_res_module_forward(module, point_d)
            assert out is point_d
        else:
            out, _ = torch_mask_res_module(net_d, temperature, point_d, sizes, ratio, None if which == "torch" else runs["hip"][0].non_leaf)
        (out.feat * g.to(DEV, dtype)).sum().backward()
        runs[which] = (out, net_d)
    hip, tor = runs["hip"][0], runs["torch"][0]
    assert set(D.MASK_RES_KEYS) <= set(hip) and set(hip) == set(tor)
    assert_cut_is_untied(tor.prob, sizes, ratio)
    for key in D.MASK_RES_KEYS + ("feat",):
        assert hip[key].dtype == tor[key].dtype and hip[key].shape == tor[key].shape, key
    for key in ("non_leaf", "leaf", "non_leaf_offset", "leaf_offset"):
        assert torch.equal(hip[key], tor[key]), key
    assert torch.equal(hip.feat, point.feat.to(DEV) * hip.non_leaf[:, None])
    grad_bar([runs[w][1] for w in ("hip", "torch", "ref")], f"MaskResModule/{sizes}")
    unchanged = D.mask_res_module_forward(types.SimpleNamespace(non_leaf_ratio=1.0), to_device(net, point, torch.float32)[1])
    assert all(unchanged[key] is None for key in D.MASK_RES_KEYS)
