"""CPU checks of tests/gemm_cases.py: the restated launch rules give the plans the GPU tests were written for, the operands are what they
claim to be, and the exactness argument holds."""
import torch

import gemm_cases as GC


def test_v1_plans():
    for m, n, k, residual, plan in GC.V1_SHAPES:
        assert GC.v1_plan(m, n, k, residual) == plan, (m, n, k, residual)
        assert k % 4 == 0 and k <= GC.MAX_K
    # each limit of the split from both sides
    assert GC.v1_plan(1984, 1024, 2052)[1] == 2 and GC.cdiv(1984, 64) * GC.cdiv(1024, 64) == 496
    assert GC.v1_plan(2048, 1024, 2052)[1] == 1 and GC.cdiv(2048, 64) * GC.cdiv(1024, 64) == 512
    assert GC.v1_plan(100, 64, 2048)[1] == 2 and GC.v1_plan(100, 64, 2044)[1] == 1
    assert GC.v1_plan(100, 64, 2048, residual=True)[1] == 1 and GC.v1_plan(70, 130, 2048)[1] == 1
    assert GC.slab_runs(2052, 2) == [33, 32] and 2052 % 32 == 4
    # <4,4> from 192 tiles of 128 x 128
    assert GC.v1_plan(24449, 100, 36) == ('4x4', 1) and GC.cdiv(24449, 128) == 192
    assert GC.v1_plan(24448, 100, 36) == ('2x2', 1)
    assert GC.cdiv(12200, 128) * GC.cdiv(130, 128) == 192 and 12200 % 128 and 130 % 128 and 68 % 32
    assert {plan for *_, plan in GC.V1_SHAPES} == {('2x2', 1), ('2x2', 2), ('4x4', 1)}


def test_v2_plans():
    for m, n, k, slices, runs in GC.V2_SHAPES:
        assert GC.v2_slices(m, n, k) == slices, (m, n, k)
        assert GC.v2_workspace(m, n, k) == slices * m * n * 4
        if slices:
            assert GC.slab_runs(k, slices) == runs and sum(runs) == k // 32 and min(runs) > 0
    assert {s for *_, s, _ in GC.V2_SHAPES} == {0, 1, 2, 4, 16}
    runs = GC.slab_runs(2080, 4)
    assert {r % 2 for r in runs} == {0, 1}              # odd and even slab counts: both parities of the double buffer's last slab
    assert (257 - 1) % 128 == 0 and (260 - 4) % 128 == 0
    # the box-head FC, for the record: 8 slices
    assert GC.v2_slices(1000, 1024, 12544) == 8


def test_operands_are_small_position_dependent_integers():
    a, bt, bias, res = GC.operands(130, 68, 2052)
    assert a.shape == (130, 2052) and bt.shape == (68, 2052) and bias.shape == (68,) and res.shape == (130, 68)
    for t, lim in ((a, 3), (bt, 3), (bias, 8), (res, 8)):
        assert t.dtype == torch.float32 and torch.equal(t, t.round()) and float(t.min()) == -lim and float(t.max()) == lim
    # no two rows, and no two slabs of a row, are equal: a kernel that reads a wrong row or slab changes the product
    assert len({tuple(r.tolist()) for r in a}) == 130 and len({tuple(r.tolist()) for r in bt}) == 68
    slabs = a[:, :2048].view(130, 64, 32)
    assert all(len({tuple(s.tolist()) for s in row}) == 64 for row in slabs[:4])
    # the float64 product is the int64 product, and every partial sum a float32 kernel can form is below 2^24
    exp = GC.exact_product(a, bt, bias, res)
    assert torch.equal(exp, (a.long() @ bt.long().t() + bias.long() + res.long()).double())
    assert GC.MAX_K * 9 + 16 < 2 ** 24
    assert torch.equal(exp.float().double(), exp)
    r = GC.exact_product(a, bt, bias, None, relu=True)
    assert 0.2 < float((r == 0).double().mean()) < 0.8          # the ReLU cuts a real share


def test_float_bound():
    g = torch.Generator().manual_seed(1)
    a, bt = torch.randn((5, 64), generator=g), torch.randn((3, 64), generator=g) / 8
    b = GC.float_bound(a, bt, None, None, 1)
    assert b.shape == (5, 3) and b.dtype == torch.float64
    assert abs(GC.gamma(131) - 131 * 2.0 ** -24) < 1e-9 and GC.gamma(131) > 131 * 2.0 ** -24
    # a float32 dot product in any order lies inside the bound
    got = (a @ bt.t()).double()
    assert bool(((got - a.double() @ bt.double().t()).abs() <= b).all())
