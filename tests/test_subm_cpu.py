"""CPU: the two restatements of the submanifold convolution agree, the table's mirror identity holds exactly where the
backward relies on it, and the `spconv` drop-in has the surface the reference's point decoder touches."""
import numpy as np
import pytest
import torch
from torch import nn

import subm_ref as R
from subm_cases import by_name, cases

DENSE = [c for c in cases() if c.dense_ok]


@pytest.mark.parametrize("case", DENSE, ids=repr)
def test_table_model_equals_dense_truth(case):
    nbr, rep = R.table_model(case.indices, case.shape, case.batch, case.ksize)
    assert (rep == np.arange(case.N)).all()
    tab = R.table_all(nbr, case.feat, case.weight, case.bias, case.grad_out)
    den = R.dense_all(case.indices, case.shape, case.batch, case.ksize, case.feat, case.weight, case.bias, case.grad_out)
    for name in ("out", "grad_feat", "grad_weight", "grad_bias"):
        a, b = tab[name], den[name]
        assert a.shape == b.shape
        # two f64 summation orders of at most N * K * C terms each
        tol = 1e-12 * max(1.0, float(b.abs().max()) if b.numel() else 0.0)
        assert float((a - b).abs().max()) <= tol if a.numel() else True, name


def test_cases_cover_what_they_claim():
    names = {c.name for c in cases()}
    assert {c.N for c in cases()} >= {0, 1, 63, 64, 65, 1500}
    assert all(max(c.shape) <= 24 for c in cases())
    assert {(c.cin, c.cout) for c in cases()} == {(16, 32), (40, 24), (160, 160)}
    assert {c.ksize for c in cases()} == {(3, 3, 3), (5, 5, 5), (1, 3, 5)}
    assert any(len(set(c.shape)) == 3 for c in cases()) and any(c.slice_of for c in cases())
    nbr, _ = R.table_model(by_name("isolated").indices, (24, 24, 24), 1, (3, 3, 3))
    assert (nbr[13] >= 0).all() and (np.delete(nbr, 13, 0) == -1).all()          # only the centre tap fires
    nbr, _ = R.table_model(by_name("full_block_c160").indices, (8, 6, 9), 1, (3, 3, 3))
    assert all((nbr[k] >= 0).any() for k in range(27))                            # every tap fires
    two = by_name("two_batches")
    nbr, _ = R.table_model(two.indices, two.shape, two.batch, two.ksize)
    src, dst = np.nonzero(nbr >= 0)[1], nbr[nbr >= 0]
    assert (two.indices[src, 0] == two.indices[dst, 0]).all()                     # the batches do not see each other
    f = by_name("faces_k5")
    for d in range(3):
        assert {0, f.shape[d] - 1} <= set(f.indices[:, 1 + d].tolist())
    sh = by_name("shared_2_5")
    _, rep = R.table_model(sh.indices, sh.shape, sh.batch, sh.ksize)
    assert sorted(set(np.bincount(rep)[np.bincount(rep) > 0].tolist())) == [1, 2, 5]
    _, rep = R.table_model(by_name("shared_all").indices, (4, 4, 4), 1, (3, 3, 3))
    assert (rep == 0).all()
    o = by_name("out_of_range")
    nbr, rep = R.table_model(o.indices, o.shape, o.batch, o.ksize)
    bad = [i for i in range(o.N) if o.indices[i, 0] >= 1 or (o.indices[i, 1:] < 0).any() or (o.indices[i, 1:] >= 5).any()]
    assert len(bad) == 3 and (nbr[:, bad] == -1).all() and not np.isin(nbr, bad).any() and (rep[bad] == bad).all()
    assert "n0" in names


def test_shared_voxel_sites_get_identical_rows_and_the_lowest_index_wins():
    c = by_name("shared_2_5")
    nbr, rep = R.table_model(c.indices, c.shape, c.batch, c.ksize)
    out = R.table_all(nbr, c.feat, c.weight, c.bias)["out"]
    assert (rep <= np.arange(c.N)).all() and (rep[rep] == rep).all()
    assert torch.equal(out, out[torch.as_tensor(rep).long()])
    assert (nbr[nbr >= 0] == rep[nbr[nbr >= 0]]).all()          # a lookup only ever answers a representative


@pytest.mark.parametrize("name", ["n1500", "two_batches", "faces_k135", "shared_2_5", "out_of_range", "full_block_k135"])
def test_mirror_identity_holds_among_representatives(name):
    c = by_name(name)
    nbr, rep = R.table_model(c.indices, c.shape, c.batch, c.ksize)
    K = nbr.shape[0]
    is_rep = rep == np.arange(c.N)
    for k in range(K):
        for i in np.nonzero(is_rep & (nbr[k] >= 0))[0]:
            assert nbr[K - 1 - k, nbr[k, i]] == i
    if not is_rep.all():       # ... and breaks for a site that is not one: its neighbours point back at its representative
        i = int(np.nonzero(~is_rep)[0][0])
        k = next(k for k in range(K) if nbr[k, i] >= 0)
        assert nbr[K - 1 - k, nbr[k, i]] == rep[i] != i


def test_drop_in_surface_and_parameters():
    import spconv.pytorch as spconv
    from generativedensification_amd import sparse_conv as S

    assert spconv.SubMConv3d is S.SubMConv3d and spconv.SparseConvTensor is S.SparseConvTensor
    assert issubclass(spconv.SubMConv3d, spconv.SparseModule) and issubclass(spconv.SparseModule, nn.Module)
    torch.manual_seed(0)
    m = spconv.SubMConv3d(16, 32, kernel_size=3, bias=True, indice_key="stage0")
    sd = m.state_dict()
    assert list(sd) == ["weight", "bias"] and sd["weight"].shape == (32, 3, 3, 3, 16) and sd["bias"].shape == (32,)
    bound = 1 / np.sqrt(16 * 27)                       # nn.Conv3d's own initialisation: U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
    assert float(m.weight.detach().abs().max()) <= bound and float(m.weight.detach().abs().max()) > 0.9 * bound
    assert float(m.bias.detach().abs().max()) <= bound and float(m.weight.detach().std()) == pytest.approx(bound / np.sqrt(3), rel=0.05)
    assert list(spconv.SubMConv3d(16, 32, (1, 3, 5), bias=False, padding=1).state_dict()) == ["weight"]
    assert spconv.modules.is_spconv_module(m) and not spconv.modules.is_spconv_module(nn.Linear(4, 4))
    for kw in (dict(stride=2), dict(dilation=2), dict(groups=2), dict(kernel_size=2), dict(kernel_size=7), dict(algo=1)):
        args = dict(in_channels=16, out_channels=16, kernel_size=3)
        args.update(kw)
        with pytest.raises(NotImplementedError):
            spconv.SubMConv3d(**args)
    with pytest.raises(NotImplementedError):
        spconv.SubMConv3d(12, 16, 3)


def test_tensor_container_and_cpu_refusal():
    import spconv.pytorch as spconv

    idx = torch.tensor([[0, 1, 2, 3], [0, 1, 2, 4]], dtype=torch.int32)
    x = spconv.SparseConvTensor(features=torch.randn(2, 16), indices=idx, spatial_shape=[8, 8, 8], batch_size=1)
    assert x.spatial_shape == [8, 8, 8] and x.batch_size == 1 and x.indices is idx
    y = x.replace_feature(torch.zeros(2, 32))
    assert y.indice_dict is x.indice_dict and y.indices is idx and y.features.shape == (2, 32) and x.features.shape == (2, 16)
    y.indice_dict["stage0"] = "table"
    assert x.indice_dict["stage0"] == "table"
    with pytest.raises(ValueError):
        spconv.SparseConvTensor(torch.randn(2, 16), idx.long(), [8, 8, 8], 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spconv.SubMConv3d(16, 32, 3)(spconv.SparseConvTensor(torch.randn(2, 16), idx, [8, 8, 8], 1))
    from generativedensification_amd.sparse_conv import build_table
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        build_table(idx, [8, 8, 8], 1, 3)


def test_argument_refusals_of_the_abi_without_a_gpu():
    import ctypes as C
    from generativedensification_amd import _lib as L

    lib = L.load()
    assert lib.gdr_subm_table_bytes(-1) == 0 and b"subm_table_bytes" in lib.gdr_last_error()
    assert lib.gdr_subm_table_bytes(1000) >= 3 * 8000 + lib.gdr_serial_sort_bytes(1, 1000)
    shape, ks = (C.c_int32 * 3)(8, 8, 8), (C.c_int32 * 3)(3, 3, 3)
    fake = 0x10000000        # never dereferenced: every call below is refused, or N = 0
    assert lib.gdr_subm_build_table(None, 0, shape, 1, ks, None, 0, None, None, None, None) == 0      # N = 0: no launch
    assert lib.gdr_subm_build_table(fake, 10, shape, 1, (C.c_int32 * 3)(3, 2, 3), fake, 1 << 20, fake, fake, fake, None) == -1
    assert b"kernel size" in lib.gdr_last_error()
    assert lib.gdr_subm_build_table(fake, 10, shape, 0, ks, fake, 1 << 20, fake, fake, fake, None) == -1
    assert lib.gdr_subm_build_table(fake, 10, shape, 1, ks, fake, 16, fake, fake, fake, None) == L.GDR_ERR_WORKSPACE
    a = L.GdrSubmArgs(0, 16, 32, 27, 2, 0)
    assert lib.gdr_subm_conv_forward(C.byref(a), None, 16, None, None, None, None, None) == 0          # N = 0
    assert lib.gdr_subm_conv_backward(C.byref(a), None, None, 16, None, None, None, None, None, 0, None, None, None, None) == 0
    for bad in (L.GdrSubmArgs(10, 12, 32, 27, 2, 0), L.GdrSubmArgs(10, 16, 520, 27, 2, 0), L.GdrSubmArgs(10, 16, 32, 126, 2, 0),
                L.GdrSubmArgs(10, 16, 32, 27, 3, 0), L.GdrSubmArgs(-1, 16, 32, 27, 0, 0)):
        assert lib.gdr_subm_conv_forward(C.byref(bad), fake, 16, fake, fake, None, fake, None) == -1
        assert lib.gdr_subm_backward_bytes(C.byref(bad)) == 0
    ok = L.GdrSubmArgs(1000, 160, 160, 27, 0, 0)
    assert lib.gdr_subm_backward_bytes(C.byref(ok)) >= 2 * 1000 * 160 * 2 + 27 * 160 * 160 * 2
    assert lib.gdr_subm_conv_forward(C.byref(ok), fake, 100, fake, fake, None, fake, None) == -1 and b"stride" in lib.gdr_last_error()
    assert lib.gdr_subm_conv_backward(C.byref(ok), fake, fake, 160, fake, fake, fake, fake, fake, 64, fake, fake, fake,
                                      None) == L.GDR_ERR_WORKSPACE


def test_point_sequential_uses_of_the_package():
    """The three ways PointSequential.forward (lightning/point_decoder/utils/modules.py, which imports pytorch_lightning and
    cannot be loaded here) touches the package, restated: an spconv module on a Point's sparse_conv_feat, a torch module on a
    Point followed by replace_feature, and a torch module on a bare SparseConvTensor."""
    import spconv.pytorch as spconv

    class Scale(spconv.SparseModule):          # a stand-in sparse module: the convolution itself needs the GPU
        def forward(self, x):
            return x.replace_feature(x.features * 2)

    class Point(dict):
        __getattr__ = dict.__getitem__
        __setattr__ = dict.__setitem__

    def forward(modules, input):
        for module in modules:
            if spconv.modules.is_spconv_module(module):
                if isinstance(input, Point):
                    input.sparse_conv_feat = module(input.sparse_conv_feat)
                    input.feat = input.sparse_conv_feat.features
                else:
                    input = module(input)
            elif isinstance(input, Point):
                input.feat = module(input.feat)
                if "sparse_conv_feat" in input.keys():
                    input.sparse_conv_feat = input.sparse_conv_feat.replace_feature(input.feat)
            elif isinstance(input, spconv.SparseConvTensor):
                if input.indices.shape[0] != 0:
                    input = input.replace_feature(module(input.features))
            else:
                input = module(input)
        return input

    idx = torch.tensor([[0, 1, 2, 3], [0, 1, 2, 4], [0, 0, 0, 0]], dtype=torch.int32)
    feat = torch.arange(3 * 16, dtype=torch.float32).reshape(3, 16)
    st = spconv.SparseConvTensor(features=feat, indices=idx, spatial_shape=[8, 8, 8], batch_size=1)
    lin = nn.Linear(16, 16)
    p = forward([Scale(), lin], Point(feat=feat, sparse_conv_feat=st))
    assert torch.equal(p.feat, lin(feat * 2)) and p.sparse_conv_feat.features is p.feat
    assert p.sparse_conv_feat.indice_dict is st.indice_dict
    out = forward([Scale(), nn.ReLU()], st)
    assert isinstance(out, spconv.SparseConvTensor) and torch.equal(out.features, feat * 2)
    empty = spconv.SparseConvTensor(torch.zeros(0, 16), idx[:0], [8, 8, 8], 1)
    assert forward([lin], empty) is empty
