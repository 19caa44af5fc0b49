"""tmf_wmrb_scores7 - item runs on the slice-major grid (one workgroup per (item slice, group of 256 users) chunk, the group's rows
in LDS, one load of a row of V for all users of the group that need it; csrc/tmf_wmrb.hip, _engine.Scores7Plan) - against
tmf_wmrb_scores3 and an fp64 product.  Both compute sp[u, s] = <U[u], V[R[u, s]]> and p[k] = <U[u_k], V[j_k]>; they differ in the
order of the fp32 sum inside a dot product only: equal to rounding on real data, bit for bit on dyadic data - and then the whole
epoch (hinge, gradients, fresh Adam) is bit-identical too."""
import os

import numpy as np
import pytest
import torch

from conftest import assert_step
from test_gpu_scores5 import CASES, problem

pytestmark = pytest.mark.gpu

F32_CASES = [c for c in CASES if c[5] is torch.float32 and 65 <= c[2] <= 128]   # the shapes the kernel exists for


@pytest.fixture(scope='module')
def eng():
    from teamoflow_amd import _engine, _lib
    _lib.get()
    return _engine


def make_state(eng, monkeypatch, s7, idx, val, R, U, V, m, n, r, dtype, slices, slice_bytes=None, slots=None):
    monkeypatch.setenv('TMF_SCORES5', '0')
    monkeypatch.setenv('TMF_SCORES6', '0')
    monkeypatch.setenv('TMF_SCORES7', '1' if s7 else '0')
    for name, v in (('TMF_S7_SLICE_BYTES', slice_bytes), ('TMF_S7_SLOTS', slots)):
        if v:
            monkeypatch.setenv(name, str(v))
        else:
            monkeypatch.delenv(name, raising=False)
    plan = eng.InteractionPlan(idx, val, m, n)
    wplan = eng.WmrbPlan(plan, R, item_slices=slices, n_components=r, sliced=True)
    st = eng.TrainState(U, V, plan, r, wplan, dtype=dtype)
    return plan, wplan, st


def epoch(eng, monkeypatch, s7, idx, val, R, U, V, m, n, r, S, dtype, slices, slice_bytes=None, slots=None, pairs=None):
    plan, wplan, st = make_state(eng, monkeypatch, s7, idx, val, R, U, V, m, n, r, dtype, slices, slice_bytes, slots)
    assert (wplan.s7 is not None) == s7 and wplan.s5 is None and wplan.s6 is None
    loss = torch.zeros(1, dtype=torch.float64, device=idx.device)
    eng.epoch_wmrb(st, eng.adam_constants(0.05), n / S, loss, pairs=pairs or 'hinge')
    torch.cuda.synchronize()
    return dict(sp=st.sp.clone(), pk=st.pk.clone(), U=st.U_nxt.float().clone(), V=st.V_nxt.float().clone(), loss=float(loss),
                D=wplan.D.clone(), delta=wplan.delta.clone(), plan=plan, wplan=wplan, st=st)


def check_against_fp64(b, r):
    st, pl = b['st'], b['plan']
    U64, V64 = st.U[:, :r].double(), st.V[:, :r].double()
    want = torch.einsum('ur,usr->us', U64, V64[b['wplan'].R.long()])
    assert float((b['sp'].double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    wantp = (U64[pl.user_of.long()] * V64[pl.col_u.long()]).sum(1)
    if wantp.numel():
        assert float((b['pk'].double() - wantp).abs().max()) <= 1e-5 * float(want.abs().max())


@pytest.mark.parametrize('m,n,r,S,nnz,dtype,slices', F32_CASES + [(33, 5000, 128, 700, 4000, torch.float32, 2)])
def test_scores7_equals_scores3_to_rounding_and_does_not_depend_on_the_chunking(eng, monkeypatch, m, n, r, S, nnz, dtype, slices):
    idx, val, R, U, V = problem(m, n, r, S, nnz, seed=m + n)
    a = epoch(eng, monkeypatch, False, idx, val, R, U, V, m, n, r, S, dtype, slices)
    # slices of 37 rows and sub-chunks of 64 slots: many sub-chunks, empty chunks, flushes of a few slots
    b = epoch(eng, monkeypatch, True, idx, val, R, U, V, m, n, r, S, dtype, slices, slice_bytes=37 * 512, slots=64)
    s7 = b['wplan'].s7
    assert s7.slots == 64 and s7.n_slices >= n // 37 - 1 and s7.n_sub >= s7.n_entries // 64
    scale = float(a['sp'].abs().max())
    assert float((a['sp'] - b['sp']).abs().max()) <= 2e-6 * scale
    assert float((a['pk'] - b['pk']).abs().max()) <= 2e-6 * scale
    assert abs(a['loss'] - b['loss']) <= 1e-6 * abs(a['loss'])
    check_against_fp64(b, r)
    # the defaults (one 4 MB slice for these small catalogs, full sub-chunks) give the same numbers bit for bit: a score does not
    # depend on the chunk, the sub-chunk or the step it is computed in
    c = epoch(eng, monkeypatch, True, idx, val, R, U, V, m, n, r, S, dtype, slices)
    assert c['wplan'].s7.slots == eng._lib.load_library().tmf_wmrb_scores7_slots()
    assert torch.equal(b['sp'], c['sp']) and torch.equal(b['pk'], c['pk'])


@pytest.mark.parametrize('m,n,r,S,nnz,dtype,slices', [CASES[0], CASES[1]])
def test_scores7_epoch_is_bit_identical_on_dyadic_tables(eng, monkeypatch, m, n, r, S, nnz, dtype, slices):
    idx, val, R, U, V = problem(m, n, r, S, nnz, seed=5 * m + n, dyadic=True)
    a = epoch(eng, monkeypatch, False, idx, val, R, U, V, m, n, r, S, dtype, slices)
    b = epoch(eng, monkeypatch, True, idx, val, R, U, V, m, n, r, S, dtype, slices, slice_bytes=100 * 512)
    for k in ('sp', 'pk', 'D', 'delta', 'U', 'V'):
        assert torch.equal(a[k], b[k]), k
    assert a['loss'] == b['loss']


@pytest.mark.parametrize('m', [70, 1])
def test_scores7_run_lengths(eng, monkeypatch, m):
    """n = 40, S = 30: every item is needed by many users of the one group (fewer than 256 users in it); the first items get runs
    of exactly K, K + 1 and 2 K + 1 users.  Bit for bit against scores3 on dyadic tables, to rounding against fp64."""
    n, r, S, K = 40, 128, 30, 4
    g = torch.Generator().manual_seed(3 + m)
    # negatives: user u draws from items 3 .. n - 1 only, plus item 0 for u < K, item 1 for u < K + 1, item 2 for u < 2 K + 1
    R = torch.stack([torch.randperm(n - 3, generator=g)[:S] + 3 for _ in range(m)]).to(torch.int32)
    for item, users in ((0, K), (1, K + 1), (2, 2 * K + 1)):
        R[:min(users, m), item] = item
    idx = torch.tensor([[u, 3 + (7 * u) % (n - 3)] for u in range(m) if u % 5 != 2] or [[0, 5]])
    val = torch.ones(idx.shape[0])
    counts = torch.bincount(R.reshape(-1).long(), minlength=n)
    if m == 70:
        assert counts[:3].tolist() == [K, K + 1, 2 * K + 1]
    for dyadic in (True, False):
        U = (torch.randint(-8, 9, (m, r), generator=g).float() / 8) if dyadic else torch.randn(m, r, generator=g) * 0.3
        V = (torch.randint(-8, 9, (n, r), generator=g).float() / 8) if dyadic else torch.randn(n, r, generator=g) * 0.3
        args = [x.cuda() for x in (idx, val, R, U, V)] + [m, n, r, S, torch.float32, 1]
        a = epoch(eng, monkeypatch, False, *args)
        b = epoch(eng, monkeypatch, True, *args)
        s7 = b['wplan'].s7
        assert s7.n_groups == 1 and s7.n_steps < s7.n_entries or m == 1
        if dyadic:
            for k in ('sp', 'pk', 'D', 'delta', 'U', 'V'):
                assert torch.equal(a[k], b[k]), k
        else:
            scale = float(a['sp'].abs().max())
            assert float((a['sp'] - b['sp']).abs().max()) <= 2e-6 * scale and float((a['pk'] - b['pk']).abs().max()) <= 2e-6 * scale
            check_against_fp64(b, r)


def test_scores7_writes_every_score_and_nothing_else(eng, monkeypatch):
    """sp and pk prefilled with NaN: every element is finite afterwards; a guard region behind each buffer stays untouched."""
    from teamoflow_amd import _lib
    lib = _lib.get()
    m, n, r, S = 300, 2000, 128, 50
    idx, val, R, U, V = problem(m, n, r, S, 5000, seed=21)
    plan, wplan, st = make_state(eng, monkeypatch, True, idx, val, R, U, V, m, n, r, torch.float32, 2, slice_bytes=300 * 512, slots=512)
    s7, G = wplan.s7, 4096
    assert s7 is not None
    sp = torch.full((m * S + G,), float('nan'), device='cuda')
    pk = torch.full((plan.nnz + G,), float('nan'), device='cuda')
    sp[m * S:] = 12345.0
    pk[plan.nnz:] = 54321.0
    _lib.check(lib.tmf_wmrb_scores7_f32(_lib.ptr(s7.steps), _lib.ptr(s7.place), _lib.ptr(s7.sub_step), _lib.ptr(s7.sub_place),
                                        _lib.ptr(s7.chunk_sub), s7.n_groups, s7.n_slices, m, n, _lib.ptr(st.U), _lib.ptr(st.V),
                                        _lib.ptr(sp), _lib.ptr(pk), r, _lib.stream_ptr()), lib)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(sp[:m * S]).all()) and bool(torch.isfinite(pk[:plan.nnz]).all())
    assert bool((sp[m * S:] == 12345.0).all()) and bool((pk[plan.nnz:] == 54321.0).all())
    U64, V64 = st.U[:, :r].double(), st.V[:, :r].double()
    want = torch.einsum('ur,usr->us', U64, V64[wplan.R.long()])
    assert float((sp[:m * S].view(m, S).double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_scores7_one_step_against_the_fp64_closed_form(eng, monkeypatch):
    from oracle import sparse_ref as SR
    m, n, r, S, lr = 600, 900, 128, 48, 0.05
    idx, val, R, U, V = problem(m, n, r, S, 12000, seed=77)
    b = epoch(eng, monkeypatch, True, idx, val, R, U, V, m, n, r, S, torch.float32, 2, slice_bytes=64 * 512)
    U64, V64 = U.cpu().numpy().astype(np.float64), V.cpu().numpy().astype(np.float64)
    i_np, v_np, R_np = idx.cpu().numpy(), val.cpu().numpy().astype(np.float64), R.cpu().numpy().astype(np.int64)
    _, _, mean, t = SR.wmrb_epoch(U64, V64, i_np, v_np, R_np, n, S, lr)
    sl = SR.wmrb_slack(U64, V64, i_np, v_np, R_np, n, S)
    n_pos = int((val > 0).sum())
    assert abs(b['loss'] / n_pos - mean) <= 1e-5 * abs(mean)
    assert_step(b['U'][:, :r].cpu().numpy(), U64, t['gU'], lr, what='scores7 U', slack=sl['gU'])
    assert_step(b['V'][:, :r].cpu().numpy(), V64, t['gV'], lr, what='scores7 V', slack=sl['gV'])


def test_scores7_bpr_step_equals_the_scores3_path(eng, monkeypatch):
    """One BPR epoch (tmf_bpr_pairs in the hinge kernel's place) through scores7 against the same through scores3: bit for bit on
    dyadic tables."""
    m, n, r, S = 500, 1200, 128, 32
    idx, val, R, U, V = problem(m, n, r, S, 6000, seed=13, dyadic=True)
    a = epoch(eng, monkeypatch, False, idx, val, R, U, V, m, n, r, S, torch.float32, 2, pairs='bpr')
    b = epoch(eng, monkeypatch, True, idx, val, R, U, V, m, n, r, S, torch.float32, 2, slice_bytes=200 * 512, pairs='bpr')
    for k in ('sp', 'pk', 'D', 'delta', 'U', 'V'):
        assert torch.equal(a[k], b[k]), k
    assert a['loss'] == b['loss']


def test_scores7_default_falls_back_when_the_streams_do_not_fit(eng, monkeypatch):
    """The default construction that runs out of memory leaves the pass with scores3; a forced one raises."""
    m, n, r, S = 300, 2000, 128, 50
    idx, val, R, U, V = problem(m, n, r, S, 5000, seed=4)

    def no_memory(*a, **k):
        raise torch.OutOfMemoryError('streams of tmf_wmrb_scores7')
    rows = tuple(f._replace(plan=no_memory) if f.name == 'scores7' else f for f in eng.SCORES_FORMS)
    monkeypatch.setattr(eng, 'SCORES_FORMS', rows)
    real = eng.scores_form   # scores7 at this small shape, as the default unless its switch forces it; behind it, the rows' own answers
    monkeypatch.setattr(eng, 'scores_form', lambda *a, after=None, **k: real(*a, after=after, **k) if after else
                        ('scores7', os.environ.get('TMF_SCORES7') == '1'))
    for name in ('TMF_SCORES5', 'TMF_SCORES6', 'TMF_SCORES7'):
        monkeypatch.delenv(name, raising=False)
    plan = eng.InteractionPlan(idx, val, m, n)
    wplan = eng.WmrbPlan(plan, R, item_slices=2, n_components=r, sliced=True)
    st = eng.TrainState(U, V, plan, r, wplan)
    assert wplan.s7 is None and wplan.s6 is None and wplan.s5 is None
    loss = torch.zeros(1, dtype=torch.float64, device='cuda')
    eng.epoch_wmrb(st, eng.adam_constants(0.05), n / S, loss)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))
    monkeypatch.setenv('TMF_SCORES7', '1')
    with pytest.raises(torch.OutOfMemoryError):
        eng.TrainState(U, V, plan, r, eng.WmrbPlan(plan, R, item_slices=2, n_components=r, sliced=True))
