"""Host: the reverse loop's options record (ldm_amd.engine.LoopOptions) on CPU tensors, with every option set: what
cut() slices, what fill() writes into the C argument struct, and what the prepare phase is keyed on.  The fields are
enumerated from the class, so one added later is covered (and fails here until it is sliced or declared shared)."""
import types

import pytest
import torch

B, C, H, W, N, R = 4, 32, 16, 64, 3, 2
SHARED = {"keep_coef", "seam_cols", "S5", "S6", "refs"}        # what cut() carries over instead of slicing
# ldm_sample_args fields that are not options: the call's own operands
NOT_OPTIONS = {"solver", "nsteps", "eta", "S5", "S6", "refs", "seam_cols", "x", "t_table", "coef_table", "x0_logs",
               "eps_logs", "log_step_stride", "workspace", "stream"}


@pytest.fixture()
def engine(monkeypatch):
    """What check() reads of an engine, and CPU tensors let through the device check (layout checks only)."""
    from ldm_amd import _lib as L
    from ldm_amd import ops
    from ldm_amd.engine import UNetEngine
    monkeypatch.setattr(ops, "require_device", lambda *a, **k: None)
    return types.SimpleNamespace(fold=True, fold_applies=UNetEngine.fold_applies,
                                 shape=lambda b, c, h, w: L.UNetShape(b, c, h, w, 64))


def full_record(engine, seam_cols=0):
    from ldm_amd.engine import LoopOptions
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.rand(*s, generator=g)      # noqa: E731
    x = r(B, C, H, W)
    s5, s6 = r(B, 256, R * H // 4, W // 4), r(B, 512, R * H // 8, W // 8)
    S5, S6 = R * H * W // 16, R * H * W // 64
    o = LoopOptions(x, N, s5, s6, key_bias5=r(B, S5), key_bias6=r(B, S6),
                    base=(r(*s5.shape), r(*s6.shape), r(B, S5), r(B, S6)), guidance_scale=torch.tensor([2.0, 0.5, 1.0, -1.0]),
                    keep=(r(B, C, H, W), r(B, C, H, W), r(B, H, W), r(N, 2)), ref_bias5=r(B, H * W // 16, R),
                    ref_bias6=r(B, H * W // 64, R), seam_cols=seam_cols)
    o.check(engine, x, N)
    return x, o


def plain_record(engine):
    from ldm_amd.engine import LoopOptions
    x = torch.zeros(B, C, H, W)
    o = LoopOptions(x, N, torch.zeros(B, 256, H // 4, W // 4), torch.zeros(B, 512, H // 8, W // 8))
    o.check(engine, x, N)
    return o


def test_cut_slices_every_per_sample_field(engine):
    from ldm_amd.engine import LoopOptions
    _, o = full_record(engine)
    c = o.cut(1, 3)
    assert set(LoopOptions.__slots__) >= SHARED
    for f in LoopOptions.__slots__:
        v, got = getattr(o, f), getattr(c, f)
        assert v is not None, f"{f}: the full record leaves it unset"
        if f in SHARED:
            assert got is v, f
        else:
            assert isinstance(v, torch.Tensor) and v.shape[0] == B, f
            assert tuple(got.shape) == (2,) + tuple(v.shape[1:]) and torch.equal(got, v[1:3]), f
            assert got.data_ptr() == v[1:3].data_ptr(), f"{f}: a copy, not a view"
    # a clone owns its tensors and keeps the derived counts
    k = o.clone()
    for f in LoopOptions.__slots__:
        v, got = getattr(o, f), getattr(k, f)
        if isinstance(v, torch.Tensor):
            assert torch.equal(got, v) and got.data_ptr() != v.data_ptr() and got.is_contiguous(), f
        else:
            assert got == v, f


def test_fill_sets_the_counts_and_every_option_pointer(engine):
    from ldm_amd import _lib as L
    from ldm_amd.engine import LoopOptions
    pointers = [f for f, _ in L.SampleArgs._fields_ if f not in NOT_OPTIONS]
    assert sorted(pointers) == sorted(LoopOptions.POINTERS.values())
    _, o = full_record(engine, seam_cols=2)
    a = L.SampleArgs()
    o.fill(a)
    assert (a.S5, a.S6, a.refs, a.seam_cols) == (2 * 64, 2 * 16, 2, 2)
    assert all(getattr(a, f) for f in pointers)
    assert a.key_bias5_base == o.key_bias5_base.data_ptr() and a.guide_scale == o.scale.data_ptr()
    assert a.keep == o.keep_w.data_ptr() and a.keep_coef == o.keep_coef.data_ptr()
    # a chain's struct points at its slice
    a2 = L.SampleArgs()
    o.cut(1, 3).fill(a2)
    assert a2.ref_bias5 == o.ref_bias5[1:3].data_ptr() and a2.keep_coef == a.keep_coef and a2.S5 == a.S5
    # the plain record: the maps alone
    p = L.SampleArgs()
    plain_record(engine).fill(p)
    assert (p.S5, p.S6, p.refs, p.seam_cols) == (0, 0, 0, 0) and p.s5 and p.s6
    assert not any(getattr(p, f) for f in pointers if f not in ("s5", "s6"))
    with pytest.raises(RuntimeError, match="check"):       # the counts come from check()
        x = torch.zeros(B, C, H, W)
        LoopOptions(x, N, torch.zeros(B, 256, H // 4, W // 4), torch.zeros(B, 512, H // 8, W // 8)).fill(L.SampleArgs())


def test_prepare_operands_are_the_prepare_phase_inputs(engine):
    """GraphedDDIM.replay: s5, s6, the key biases, the base maps and biases (and t_table, which the graph adds)."""
    _, o = full_record(engine)
    want = [o.s5, o.s6, o.key_bias5, o.key_bias6, o.s5_base, o.s6_base, o.key_bias5_base, o.key_bias6_base]
    got = o.prepare_operands()
    assert len(got) == len(want) and all(g is w for g, w in zip(got, want))
    for t in (o.scale, o.z0, o.n0, o.keep_w, o.keep_coef, o.ref_bias5, o.ref_bias6):
        assert not any(g is t for g in got)
    assert plain_record(engine).prepare_operands()[2:] == (None,) * 6


def test_public_keywords_rebuild_the_record(engine):
    from ldm_amd.engine import LoopOptions
    x, o = full_record(engine, seam_cols=3)
    again = LoopOptions(x, N, o.s5, o.s6, **o.public())
    for f in LoopOptions.POINTERS:
        assert torch.equal(getattr(again, f), getattr(o, f)), f
    assert again.seam_cols == 3 and plain_record(engine).public() == {}
