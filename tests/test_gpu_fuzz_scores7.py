"""The item-run scores kernel (tmf_wmrb_scores7_f32 / tmf_wmrb_scores7_fill_f32: csrc/tmf_wmrb.hip, _engine.Scores7Plan) under
random forms of every other pass, on the random problems of tests/test_fuzz_draws_cpu.py (draw_s7: any slots per sub-chunk, slices
down to one row, users around the group borders, ids repeated in a row, a user's own positive among its negatives): the assertions
of test_gpu_fuzz_forms.test_random_forms_against_the_closed_form, every score against an fp64 product, fill order against item order
and a second run of the same state bit for bit.  Then the two things no other test reaches: a scores7 grid of 2^32 work-items that
has to go out in several launches, and scores7 epochs captured into a hipGraph.  TMF_FUZZ_SEEDS=100 for a soak run."""
import os
import time

import numpy as np
import pytest
import torch

from conftest import assert_step, report_slack
from test_fuzz_draws_cpu import FORM_KEYS, draw_s7
from test_gpu_fuzz_forms import assert_epochs_are_the_closed_form, build_state, gradient_and_step_epochs, self_pair_floor
from test_gpu_scores7 import check_against_fp64

pytestmark = pytest.mark.gpu

N_SEEDS = int(os.environ.get('TMF_FUZZ_SEEDS', '24'))
NAN = float('nan')
WORST = {}


@pytest.fixture(scope='module')
def eng():
    from teamoflow_amd import _engine, _lib
    _lib.get()
    t0 = time.time()
    yield _engine
    if WORST:   # relative: sp / pk to max |sp| against fp64, the loss to the closed form's, gU / gV beyond their slack to max |g|
        report_slack(test='fuzz_scores7', seeds=N_SEEDS, seconds=round(time.time() - t0, 1), **{k: float(f'{v:.3g}') for k, v in sorted(WORST.items())})


def note(**errs):
    for k, v in errs.items():
        WORST[k] = max(WORST.get(k, 0.0), float(v))


def run(eng, st, wplan, m, n, S):
    """sp and pk filled with NaN, then the raw-gradient epoch and the stepping epoch -> everything they wrote."""
    st.sp.fill_(NAN)
    st.pk.fill_(NAN)
    loss, loss2, gU, gV = gradient_and_step_epochs(eng, st, m, n, S)
    return dict(sp=st.sp.clone(), pk=st.pk.clone(), D=wplan.D.clone(), delta=wplan.delta.clone(), gU=gU, gV=gV, U=st.U_nxt.clone(),
                V=st.V_nxt.clone(), loss=float(loss), loss2=float(loss2))


BITS = ('sp', 'pk', 'D', 'delta', 'gU', 'gV', 'U', 'V')


@pytest.mark.parametrize('seed', range(N_SEEDS))
def test_scores7_under_random_forms_against_the_closed_form(eng, monkeypatch, seed):
    m, n, r, S, idx, val, R, U, V, dtype, env = problem = draw_s7(seed)
    fill = env['TMF_S7_FILL'] == '1'
    plan, wplan, st, what = build_state(eng, monkeypatch, *problem)
    s7 = wplan.s7
    assert wplan.sliced and wplan.s5 is None and wplan.s6 is None and s7 is not None, what
    assert (s7.sub_wave is not None) == fill and (s7.sub_fill is not None) == fill, what
    assert s7.slots == int(env.get('TMF_S7_SLOTS', s7.pad_slot)) and s7.n_entries == plan.nnz + m * S, what
    if 'TMF_S7_SLICE_BYTES' in env:
        assert s7.width == -(-n // -(-n * 512 // int(env['TMF_S7_SLICE_BYTES']))), what
    else:
        assert s7.n_slices == 1, what
    a = run(eng, st, wplan, m, n, S)
    # every score was written, and is the fp64 product to rounding
    assert bool(torch.isfinite(a['sp']).all()) and bool(torch.isfinite(a['pk']).all()), what
    check_against_fp64(dict(a, st=st, plan=plan, wplan=wplan), r)
    U64, V64 = st.U[:, :r].double(), st.V[:, :r].double()
    want = torch.einsum('ur,usr->us', U64, V64[wplan.R.long()])
    scale = float(want.abs().max())
    wantp = (U64[plan.user_of.long()] * V64[plan.col_u.long()]).sum(1)
    note(sp=float((a['sp'].double() - want).abs().max()) / scale, pk=float((a['pk'].double() - wantp).abs().max()) / scale)
    loss = torch.tensor([a['loss']], dtype=torch.float64)
    note(**assert_epochs_are_the_closed_form(st, loss, torch.tensor([a['loss2']], dtype=torch.float64), a['gU'], a['gV'], m, n, r, S, idx,
                                             val, R, dtype, what))
    # the same state once more: the same bits
    b = run(eng, st, wplan, m, n, S)
    for k in BITS:
        assert torch.equal(a[k], b[k]), (k, 'second run of one state', what)
    assert a['loss'] == b['loss'] == b['loss2'], what
    # a second state in the other step order: a score has one summation tree wherever its step runs
    env2 = dict(env, TMF_S7_FILL='0' if fill else '1')
    plan2, wplan2, st2, what2 = build_state(eng, monkeypatch, m, n, r, S, idx, val, R, U, V, dtype, env2)
    assert wplan2.s7 is not None and (wplan2.s7.sub_wave is not None) == (not fill), what2
    c = run(eng, st2, wplan2, m, n, S)
    for k in BITS:
        assert torch.equal(a[k], c[k]), (k, 'fill order against item order', what)
    assert a['loss'] == c['loss'], what


@pytest.mark.parametrize('seed', range(max(6, N_SEEDS // 4)))
def test_scores7_under_random_forms_over_several_epochs_teacher_forced(eng, monkeypatch, seed):
    """Three epochs in a row on one TrainState: after every epoch the tables lie in the fresh-Adam step interval of the fp64 closed
    form evaluated at the tables the epoch STARTED from - nothing stale in sp / pk, the score buffer or the plan from the epoch before."""
    from oracle import sparse_ref as SR
    m, n, r, S, idx, val, R, U, V, dtype, env = problem = draw_s7(5000 + seed)
    plan, wplan, st, what = build_state(eng, monkeypatch, *problem)
    assert wplan.s7 is not None and wplan.s6 is None, what
    lr, adam = 0.05, eng.adam_constants(0.05)
    v64, R64 = val.astype(np.float64), R.astype(np.int64)
    rtol = 1e-5 + 5e-7 * (n / S)
    n_pos = int((val > 0).sum())
    loss = torch.zeros(3, dtype=torch.float64, device='cuda')
    for e in range(3):
        U64, V64 = st.U[:, :r].double().cpu().numpy(), st.V[:, :r].double().cpu().numpy()
        eng.epoch_wmrb(st, adam, n / S, loss[e:e + 1])
        st.swap()
        torch.cuda.synchronize()
        _, _, mean, t = SR.wmrb_epoch(U64, V64, idx, v64, R64, n, S, lr)
        sl = SR.wmrb_slack(U64, V64, idx, v64, R64, n, S)
        fU, fV = self_pair_floor(n / S, U64, V64)
        assert abs(float(loss[e]) / n_pos - mean) <= rtol * abs(mean) + 1e-12, (e, what)
        assert_step(st.U[:, :r].cpu().numpy(), U64, t['gU'], lr, rtol=rtol, what=f'epoch {e} U {what}', slack=sl['gU'] + fU)
        assert_step(st.V[:, :r].cpu().numpy(), V64, t['gV'], lr, rtol=rtol, what=f'epoch {e} V {what}', slack=sl['gV'] + fV)


def test_scores7_grid_beyond_one_launch(eng, monkeypatch):
    """A HIP launch carries fewer than 2^32 work-items.  1.1M users are 4297 groups of 1024 threads: at most 976 slices per launch,
    and slices of one row on a catalog of 2000 items make 2000 - three launches of whole slices (wmrb_scores7_impl).  Most chunks
    are empty and return at once.  On dyadic tables one epoch is the scores3 epoch bit for bit; the scores, prefilled with NaN, are
    all written and are the fp64 products.  Item order, then fill order."""
    m, n, r, S, nnz = 1_100_000, 2000, 128, 1, 1_100_000
    g = torch.Generator(device='cuda').manual_seed(7)
    u = torch.randint(0, m, (nnz,), generator=g, device='cuda')
    j = torch.randint(0, n, (nnz,), generator=g, device='cuda')
    key = torch.unique(u * n + j)
    idx = torch.stack([key // n, key % n], 1)
    val = torch.randint(-1, 6, (key.numel(),), generator=g, device='cuda').float()
    R = torch.randint(0, n, (m, S), generator=g, device='cuda').to(torch.int32)
    U = torch.randint(-8, 9, (m, r), generator=g, device='cuda').float() / 8
    V = torch.randint(-8, 9, (n, r), generator=g, device='cuda').float() / 8
    del u, j, key

    def epoch(forms):
        for k in FORM_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in dict({'TMF_SCORES5': '0', 'TMF_SCORES6': '0', 'TMF_ITEM_SLICES': '2'}, **forms).items():
            monkeypatch.setenv(k, v)
        plan = eng.InteractionPlan(idx, val, m, n)
        wplan = eng.WmrbPlan(plan, R, item_slices=2, n_components=r, sliced=True)
        st = eng.TrainState(U, V, plan, r, wplan)
        st.sp.fill_(NAN)
        st.pk.fill_(NAN)
        loss = torch.zeros(1, dtype=torch.float64, device='cuda')
        eng.epoch_wmrb(st, eng.adam_constants(0.05), n / S, loss)
        torch.cuda.synchronize()
        out = dict(sp=st.sp, pk=st.pk, D=wplan.D, delta=wplan.delta, U=st.U_nxt, V=st.V_nxt, loss=float(loss))
        return out, plan, wplan.s7

    a, plan, none = epoch({'TMF_SCORES7': '0'})
    assert none is None
    # fp64 products in user blocks
    want_sp, want_pk = torch.empty(m, S, device='cuda'), torch.empty(plan.nnz, device='cuda')
    V64 = V.double()
    for b in range(0, m, 1 << 18):
        want_sp[b:b + (1 << 18)] = torch.einsum('ur,usr->us', U[b:b + (1 << 18)].double(), V64[torch.sort(R[b:b + (1 << 18)].long(), 1)[0]]).float()
    for b in range(0, plan.nnz, 1 << 18):
        k = slice(b, b + (1 << 18))
        want_pk[k] = (U[plan.user_of[k].long()].double() * V64[plan.col_u[k].long()]).sum(1).float()
    assert torch.equal(a['sp'], want_sp) and torch.equal(a['pk'], want_pk)          # dyadic: exact in fp32, whatever the order
    for fill in ('0', '1'):
        b, _, s7 = epoch({'TMF_SCORES7': '1', 'TMF_S7_SLICE_BYTES': '512', 'TMF_S7_FILL': fill})
        assert s7 is not None and (s7.sub_wave is not None) == (fill == '1')
        assert s7.n_groups == 4297 and s7.n_slices == 2000 and s7.n_groups * s7.n_slices * 1024 >= 2 ** 32
        assert (2 ** 32 - 1) // (s7.n_groups * 1024) == 976                       # slices per launch: 976 + 976 + 48
        assert bool(torch.isfinite(b['sp']).all()) and bool(torch.isfinite(b['pk']).all())
        for k in ('sp', 'pk', 'D', 'delta', 'U', 'V'):
            assert torch.equal(a[k], b[k]), (k, fill)
        assert a['loss'] == b['loss']
        del b, s7
    del a, plan, want_sp, want_pk, V64, idx, val, R, U, V
    torch.cuda.empty_cache()


LOSSES = ('wmrb', 'bpr', 'warp', 'softmax_scaled')


@pytest.mark.parametrize('fill', ['0', '1'])
@pytest.mark.parametrize('loss', LOSSES)
def test_captured_scores7_epochs_equal_launched_epochs(monkeypatch, loss, fill):
    """fit() captures the epochs of small problems into a hipGraph: replaying it gives the bits that launching the same kernels one
    by one gives - with the scores from the item-run kernel, in item order and in fill order, under every loss that runs on it."""
    from test_bpr_cpu import bpr_problem
    from test_warp_cpu import warp_problem
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import BPRLoss, SampledSoftmaxLoss, WARPLoss, WMRBLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    m, n, r, S = 300, 400, 128, 24
    p = (warp_problem if loss == 'warp' else bpr_problem)(40 + LOSSES.index(loss), m, n, r, S, density=0.03)
    graph = dict(wmrb=WMRBLoss, bpr=BPRLoss, warp=WARPLoss, softmax_scaled=lambda: SampledSoftmaxLoss(catalog_scale=True))[loss]
    for k in FORM_KEYS:
        monkeypatch.delenv(k, raising=False)
    env = {'TMF_FORCE_SLICED': '1', 'TMF_SCORES5': '0', 'TMF_SCORES6': '0', 'TMF_SCORES7': '1', 'TMF_S7_FILL': fill, 'TMF_S7_SLICE_BYTES': str(100 * 512),
           'TMF_S7_SLOTS': '512', 'TMF_ITEM_SLICES': '3'}
    for k, v in env.items():
        monkeypatch.setenv(k, v)

    def fit(no_graph):
        if no_graph:
            monkeypatch.setenv('TMF_NO_GRAPH', '1')
        else:
            monkeypatch.delenv('TMF_NO_GRAPH', raising=False)
        model = MatrixFactorization(r, loss_graph=graph(), user_weight_graph=FixedInitializer(p['U0']), item_weight_graph=FixedInitializer(p['V0']),
                                    n_users=m, n_items=n, n_samples=S)
        model.random_ind = torch.as_tensor(p['R'])
        model.verbose = False
        model.fit(7, eye(m), eye(n), SparseInteractions(p['idx'], p['val'], (m, n)), lr=0.05)       # six captured epochs + one launched
        s7 = model._state.wplan.s7
        assert s7 is not None and (s7.sub_wave is not None) == (fill == '1') and s7.n_slices == 4 and s7.n_groups == 2 and s7.n_sub > 8
        return model
    a, b = fit(False), fit(True)
    assert a.graph_epochs_ == 6 and b.graph_epochs_ == 0, (a.graph_epochs_, b.graph_epochs_)   # one did replay a graph, the other did not
    assert len(a.loss_history_) == 7 and np.isfinite(a.loss_history_).all() and len(set(a.loss_history_)) == 7
    assert a.loss_history_ == b.loss_history_, (loss, fill, a.loss_history_, b.loss_history_)
    assert torch.equal(a.user_embedding, b.user_embedding) and torch.equal(a.item_embedding, b.item_embedding), (loss, fill)
