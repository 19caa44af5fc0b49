"""BPR, WARP and the sampled softmax (c = 1 and c = n / S) - epoch_wmrb(pairs=...) - under random forms of every pass, the scores from
tmf_wmrb_scores3, tmf_wmrb_scores6 or the item-run kernel tmf_wmrb_scores7, on the random problems of tests/test_fuzz_draws_cpu.py
(draw_pairs; its CPU tests show every tolerance used here to be reachable in fp32 and every WARP problem to be decided): the loss,
delta, D and the raw gradients against the fp64 closed forms of the losses' own tests, the tables after one step inside the
fresh-Adam interval, rows without a gradient and pad columns untouched, and - on dyadic tables - the drawn forms against the plain
ones bit for bit.  TMF_FUZZ_SEEDS=100 for a soak run."""
import os
import time

import numpy as np
import pytest
import torch

from conftest import assert_step, rel_err, report_slack
from test_fuzz_draws_cpu import FORM_KEYS, PAIR_KINDS, closed_form, draw_pairs, dyadic_pair_seed
from test_gpu_fuzz_forms import PLAIN
from test_softmax_cpu import sum_identity_gaps

pytestmark = pytest.mark.gpu

N_SEEDS = int(os.environ.get('TMF_FUZZ_SEEDS', '24'))
NAN = float('nan')
LR = 0.05
WORST = {}


@pytest.fixture(scope='module')
def eng():
    from teamoflow_amd import _engine, _lib
    _lib.get()
    t0 = time.time()
    yield _engine
    for kind, errs in sorted(WORST.items()):   # the worst relative error of every kind against its fp64 closed form
        report_slack(test='fuzz_pairs', kind=kind, seeds=N_SEEDS, seconds=round(time.time() - t0, 1),
                     **{k: float(f'{v:.3g}') for k, v in errs.items()})


def note(kind, **errs):
    mine = WORST.setdefault(kind, {})
    for k, v in errs.items():
        mine[k] = max(mine.get(k, 0.0), float(v))


def build(eng, monkeypatch, d, env, U, V):
    """The plans and the state of a fit of this loss (always the sliced user pass) under ``env``; the COO pairs in the draw's order."""
    p = d['p']
    for k in FORM_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dev, o = 'cuda', d['order']
    plan = eng.InteractionPlan(torch.tensor(p['idx'][o], device=dev), torch.tensor(p['val'][o], device=dev), p['m'], p['n'])
    wplan = eng.wmrb_plan_for(plan, torch.tensor(p['R'], device=dev), p['r'], torch.float32, force_sliced=True)
    st = eng.TrainState(torch.tensor(U, device=dev), torch.tensor(V, device=dev), plan, p['r'], wplan)
    return plan, wplan, st


def expected_forms(d):
    from teamoflow_amd import _lib
    lib, env, r = _lib.get(), d['env'], d['p']['r']
    rows4 = env['TMF_ROWS4'] == '1' and bool(lib.tmf_wsum_rows4_rows_per_group(r, 0))
    return dict(s6=d['form'] == 's6', s7=d['form'] == 's7', rows4=rows4, vrows=rows4 and env['TMF_ROWS5'] != '0',
                rs=env['TMF_ROW_STATIONARY'] == '1' and bool(lib.tmf_wmrb_gradu4_supported(r, 0)))


def forms_of(wplan, st):
    return dict(s6=wplan.s6 is not None, s7=wplan.s7 is not None, rows4=wplan.rows4, vrows=wplan.vrows is not None, rs=st.row_stationary)


def pairs_of(kind):
    return 'softmax' if kind.startswith('softmax') else kind


@pytest.mark.parametrize('seed', range(N_SEEDS))
def test_pair_losses_under_random_forms_against_the_closed_form(eng, monkeypatch, seed):
    from teamoflow_amd import _lib
    d = draw_pairs(seed)
    p, kind, c = d['p'], d['kind'], d['c']
    m, n, r, S = p['m'], p['n'], p['r'], p['S']
    plan, wplan, st = build(eng, monkeypatch, d, d['env'], p['U0'], p['V0'])
    what = dict(d['env'], seed=seed, kind=kind, c=c, m=m, n=n, r=r, S=S, nnz=len(p['val']), permuted=d['permute'], slices=wplan.n_slices,
                **forms_of(wplan, st))
    assert wplan.sliced and wplan.s5 is None and forms_of(wplan, st) == expected_forms(d), what
    if wplan.s7 is not None:
        assert (wplan.s7.sub_wave is not None) == (d['env']['TMF_S7_FILL'] == '1'), what
    adam, dev = eng.adam_constants(LR), 'cuda'
    st.sp.fill_(NAN)
    st.pk.fill_(NAN)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    gU = torch.full((m, st.ld), 7.0, device=dev)
    gV = torch.full((n, st.ld), 7.0, device=dev)
    eng.epoch_wmrb(st, adam, c, loss, item_epi=_lib.EPI_GRAD, item_out=gV, user_epi=_lib.EPI_GRAD, user_out=gU, pairs=pairs_of(kind))
    delta, D = wplan.delta.cpu().numpy(), wplan.D_in_model_order().cpu().numpy()
    loss2 = torch.zeros(1, dtype=torch.float64, device=dev)
    st.U_nxt.fill_(NAN)
    st.V_nxt.fill_(NAN)
    eng.epoch_wmrb(st, adam, c, loss2, pairs=pairs_of(kind))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(st.sp).all()) and bool(torch.isfinite(st.pk).all()), what
    assert float(loss) == float(loss2), what                                      # the two epochs read the same tables
    ref_loss, ref_delta, ref_D, ref_gU, ref_gV = closed_form(d)                  # on the row-major pairs; the plan's CSR order is row-major
    errs = dict(loss=rel_err(float(loss), ref_loss), delta=rel_err(delta, ref_delta), D=rel_err(D, ref_D),
                gU=rel_err(gU[:, :r].cpu().numpy(), ref_gU), gV=rel_err(gV[:, :r].cpu().numpy(), ref_gV))
    print(f'[fuzz pairs] {what}: ' + ' '.join(f'{k} {v:.3g}' for k, v in errs.items()))
    note(kind, **errs)
    assert max(errs.values()) < 1e-5, (errs, what)
    if kind == 'warp':      # the reference's first violators exactly
        assert np.array_equal(D != 0, ref_D != 0) and np.array_equal(delta != 0, ref_delta != 0), what
    if kind.startswith('softmax'):
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(p['idx'][:, 0], minlength=m))])
        assert all(gap <= 1e-5 * size for gap, size in sum_identity_gaps(rowptr, p['val'], delta, D)), what
    U1, V1 = st.U_nxt.cpu().numpy(), st.V_nxt.cpu().numpy()
    assert_step(U1[:, :r], p['U0'], ref_gU, LR, rtol=1e-5, what=f'U {what}')
    assert_step(V1[:, :r], p['V0'], ref_gV, LR, rtol=1e-5, what=f'V {what}')
    # a user without a positive and an item nobody stores or samples have no gradient: their rows keep their bits
    for user in (p['empty_user'], p['nonpos_user']):
        assert not gU[user].any() and np.array_equal(U1[user, :r], p['U0'][user]), (user, what)
    assert not gV[p['empty_item']].any() and np.array_equal(V1[p['empty_item'], :r], p['V0'][p['empty_item']]), what
    # pad columns: zero in the tables read, the tables written and the raw gradients
    assert st.ld >= r and not U1[:, r:].any() and not V1[:, r:].any() and not bool(st.U[:, r:].any()) and not bool(st.V[:, r:].any()), what
    assert not bool(gU[:, r:].any()) and not bool(gV[:, r:].any()), what
    assert np.isfinite(U1).all() and np.isfinite(V1).all(), what                 # every row was written


@pytest.mark.parametrize('seed', range(max(6, N_SEEDS // 4)))
def test_pair_losses_on_dyadic_tables_equal_the_plain_forms(eng, monkeypatch, seed):
    """Tables of multiples of 1/8: every score is exact in fp32 whatever the order of its sum, so the drawn forms give the scores,
    the weights and the loss of the plain forms (scores3, gradu3 + finish, lists + slab) bit for bit."""
    d = draw_pairs(dyadic_pair_seed(seed))      # every kind in turn, each on scores7 in its first case
    p, kind, c = d['p'], d['kind'], d['c']
    assert kind == PAIR_KINDS[seed % 4] and (d['form'] == 's7' or seed >= 4), d['form']
    m, n, r, S = p['m'], p['n'], p['r'], p['S']
    g = torch.Generator().manual_seed(seed)
    U = (torch.randint(-8, 9, (m, r), generator=g).float() / 8).numpy()
    V = (torch.randint(-8, 9, (n, r), generator=g).float() / 8).numpy()
    out = []
    for env in (PLAIN, d['env']):
        plan, wplan, st = build(eng, monkeypatch, d, env, U, V)
        st.sp.fill_(NAN)
        st.pk.fill_(NAN)
        loss = torch.zeros(1, dtype=torch.float64, device='cuda')
        eng.epoch_wmrb(st, eng.adam_constants(LR), c, loss, pairs=pairs_of(kind))
        torch.cuda.synchronize()
        out.append(dict(sp=st.sp.clone(), pk=st.pk.clone(), D=wplan.D.clone(), delta=wplan.delta.clone(), loss=float(loss),
                        forms=forms_of(wplan, st)))
    a, b = out
    what = dict(d['env'], seed=seed, kind=kind, m=m, n=n, r=r, S=S, **b['forms'])
    assert not any(a['forms'].values()), a['forms']
    assert b['forms'] == expected_forms(d), what
    for k in ('sp', 'pk', 'D', 'delta'):
        assert torch.equal(a[k], b[k]), (k, what)
    assert a['loss'] == b['loss'] and np.isfinite(a['loss']), what
