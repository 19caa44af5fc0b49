"""The five table losses (WMRB, BPR, WARP, k-OS WARP, sampled softmax) from a non-zero scalar item bias under random forms of every
pass - scores3 / scores6 / scores7, item slices, user blocks, rows4 / rows5, row-stationary gradU, permuted COO - on the random
problems of tests/test_fuzz_draws_cpu.py (draw_bias; its CPU tests show that the tolerances used here are reachable in fp32, that the
kinked losses' problems are decided, and that the draws hold list rows past the unrolled loop of k_item_bias_partial and further
chunks at ITEM_BIAS_CHUNK): the loss and the RAW gradients of U, V and b against tests/item_bias_ref.py (fp64 autograd of the model's
own get_loss; shares no code with the engine), the tables and b after one step inside the fresh-Adam interval, rows, items and pads
without a gradient untouched, and - on dyadic tables - the drawn forms against the plain ones bit for bit.  TMF_FUZZ_SEEDS=100 for a
soak run."""
import time

import numpy as np
import pytest
import torch

from conftest import assert_step, report_slack
from item_bias_ref import ulp32
from test_fuzz_draws_cpu import BIAS_KINDS, BIAS_RTOL, FORM_KEYS, N_BIAS_SEEDS, bias_errors, bias_reference, draw_bias
from test_gpu_fuzz_forms import PLAIN
from test_gpu_fuzz_pairs import expected_forms, forms_of

pytestmark = pytest.mark.gpu

NAN = float('nan')
LR = 0.05
WORST = {}
DYADIC_SEEDS = (0, 1, 2, 3, 4, 13)   # draw_bias seeds: round 0 is a scores7 round of every kind, one user block; 13 is k-OS WARP on scores6, a
#                                      three-column round that keeps its drawn user blocks (the test asserts that there are several)


@pytest.fixture(scope='module')
def eng():
    from teamoflow_amd import _engine, _lib
    _lib.get()
    assert set(BIAS_KINDS) == {name for name, rec in _engine.LOSSES.items() if rec.table}
    t0 = time.time()
    yield _engine
    for kind, errs in sorted(WORST.items()):   # the worst relative error of every kind against the fp64 reference
        report_slack(test='fuzz_bias', kind=kind, seeds=N_BIAS_SEEDS, rtol=BIAS_RTOL[kind], seconds=round(time.time() - t0, 1),
                     **{k: float(f'{v:.3g}') for k, v in errs.items()})


def note(kind, **errs):
    mine = WORST.setdefault(kind, {})
    for k, v in errs.items():
        mine[k] = max(mine.get(k, 0.0), float(v))


def build(eng, monkeypatch, d, env, U, V, b0):
    """The plans and the state of a fit of this loss with a scalar item bias (tests/test_gpu_item_bias.py's engine_state) under ``env``;
    the COO pairs in the draw's order."""
    p, rec = d['p'], eng.LOSSES[d['name']]
    for k in FORM_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dev, o = 'cuda', d['order']
    plan = eng.InteractionPlan(torch.tensor(p['idx'][o], device=dev), torch.tensor(p['val'][o], device=dev), p['m'], p['n'], **rec.plan_form())
    table = eng.checked_negatives(np.array(p['R']), p['m'], p['n'], dev)
    wplan = eng.wmrb_plan_for(plan, table, p['r'], force_sliced=True)
    rec.prepare(wplan, plan)
    st = eng.TrainState(torch.tensor(U, device=dev), torch.tensor(V, device=dev), plan, p['r'], wplan, item_scalar_bias=np.array(b0))
    return plan, wplan, st


@pytest.mark.parametrize('seed', range(N_BIAS_SEEDS))
def test_table_losses_with_a_bias_under_random_forms_against_fp64_autograd(eng, monkeypatch, seed):
    """Tolerance: tests/test_fuzz_draws_cpu.py's BIAS_RTOL - 1e-5, and for WMRB four times the largest error of the reference's own
    computation in float32 (2.421e-5 -> 9.684e-5: its weights move by c^2 = (n / S)^2 times a score's rounding).  In a long-list round
    gb is held to it twice: over all items, and over the items but the long one, whose gradient would otherwise set the scale."""
    from teamoflow_amd import _lib
    d = draw_bias(seed)
    p, kind, c, b0 = d['p'], d['kind'], d['c'], d['b0']
    m, n, r, S = p['m'], p['n'], p['r'], p['S']
    rec, rtol = eng.LOSSES[d['name']], BIAS_RTOL[kind]
    plan, wplan, st = build(eng, monkeypatch, d, d['env'], p['U0'], p['V0'], b0)
    ib = st.ib
    what = dict(d['env'], seed=seed, kind=kind, m=m, n=n, r=r, S=S, nnz=len(p['val']), permuted=d['permute'], slices=wplan.n_slices,
                blocks=wplan.user_chunks, n_extra=ib.n_extra, longest=int((wplan.rowptr_e[1:] - wplan.rowptr_e[:-1]).max()),
                **forms_of(wplan, st))
    assert wplan.sliced and wplan.s5 is None and ib is not None and forms_of(wplan, st) == expected_forms(d), what
    assert wplan.user_chunks == int(d['env']['TMF_USER_CHUNKS']) and ib.chunk == eng.ITEM_BIAS_CHUNK, what
    if wplan.s7 is not None:
        assert (wplan.s7.sub_wave is not None) == (d['env']['TMF_S7_FILL'] == '1'), what
    adam, dev = eng.adam_constants(LR), 'cuda'
    # epoch 1: the raw gradients of U, V and b
    st.sp.fill_(NAN)
    st.pk.fill_(NAN)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    gU = torch.full((m, st.ld), 7.0, device=dev)
    gV = torch.full((n, st.ld), 7.0, device=dev)
    ib.b_nxt[:n].fill_(7.0)
    ib.epi = _lib.EPI_GRAD
    eng.epoch_wmrb(st, adam, c, loss, item_epi=_lib.EPI_GRAD, item_out=gV, user_epi=_lib.EPI_GRAD, user_out=gU, pairs=rec.pairs)
    gb = ib.b_nxt[:n].clone()
    assert not bool(ib.b_nxt[n:].any()) and not bool(ib.b[n:].any()), what
    # epoch 2: the default epilogues, from the same tables
    loss2 = torch.zeros(1, dtype=torch.float64, device=dev)
    st.U_nxt.fill_(NAN)
    st.V_nxt.fill_(NAN)
    ib.b_nxt[:n].fill_(NAN)
    ib.epi = _lib.EPI_ADAM
    eng.epoch_wmrb(st, adam, c, loss2, pairs=rec.pairs)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(st.sp).all()) and bool(torch.isfinite(st.pk).all()), what
    assert float(loss) == float(loss2), what
    ref = bias_reference(d)
    gU, gV, gb = gU.cpu().numpy(), gV.cpu().numpy(), gb.cpu().numpy()
    errs = bias_errors(d, ref, float(loss), gU[:, :r], gV[:, :r], gb)
    assert ('gb_rest' in errs) == d['long_lists'], what
    print(f'[fuzz bias] {what}: ' + ' '.join(f'{k} {v:.3g}' for k, v in errs.items()))
    note(kind, **errs)
    assert max(errs.values()) < rtol, (errs, what)
    U1, V1, b1 = st.U_nxt.cpu().numpy(), st.V_nxt.cpu().numpy(), ib.b_nxt[:n].cpu().numpy()
    assert_step(U1[:, :r], p['U0'], ref['gU'], LR, rtol=rtol, what=f'U {what}')
    assert_step(V1[:, :r], p['V0'], ref['gV'], LR, rtol=rtol, what=f'V {what}')
    assert_step(b1, b0, ref['gb'], LR, rtol=rtol, what=f'b {what}')
    # a user without a positive and an item nobody stores or samples have no gradient: their rows and its bias keep their bits
    empty = p['empty_item']
    for user in (p['empty_user'], p['nonpos_user']):
        assert not gU[user].any() and np.array_equal(U1[user, :r], p['U0'][user]), (user, what)
    assert not gV[empty].any() and np.array_equal(V1[empty, :r], p['V0'][empty]), what
    assert gb[empty] == 0 and b1[empty] == b0[empty] and ib.value[empty].item() == b0[empty], what
    # pad columns of the tables and the padding of b / b_nxt behind n_items: zero
    assert st.ld >= r and not U1[:, r:].any() and not V1[:, r:].any() and not bool(st.U[:, r:].any()) and not bool(st.V[:, r:].any()), what
    assert not gU[:, r:].any() and not gV[:, r:].any(), what
    assert not bool(ib.b_nxt[n:].any()) and not bool(ib.b[n:].any()) and np.array_equal(ib.value.cpu().numpy(), b0), what
    assert np.isfinite(U1).all() and np.isfinite(V1).all() and np.isfinite(b1).all(), what      # every row and every bias was written


@pytest.mark.parametrize('seed', DYADIC_SEEDS)
def test_biased_losses_on_dyadic_tables_equal_the_plain_forms(eng, monkeypatch, seed):
    """Tables and a bias of multiples of 1/8: every score is exact in fp32 whatever the order of its sum, so the drawn forms give the
    scores, the weights and the loss of the plain forms (scores3, gradu3 + finish, lists + slab) bit for bit.  The raw gradient of b
    is then a sum of the SAME weights in both runs, in the fixed order of each run's user blocks: both within one rounding to fp32
    of the fp64 sum (tests/test_gpu_item_bias.py's bound)."""
    from teamoflow_amd import _lib
    d = draw_bias(seed)
    p, kind, c = d['p'], d['kind'], d['c']
    assert kind == BIAS_KINDS[seed % 5] and (d['form'] == 's7' or seed >= 5), d['form']
    m, n, r, S = p['m'], p['n'], p['r'], p['S']
    rec = eng.LOSSES[d['name']]
    g = torch.Generator().manual_seed(seed)
    U = (torch.randint(-8, 9, (m, r), generator=g).float() / 8).numpy()
    V = (torch.randint(-8, 9, (n, r), generator=g).float() / 8).numpy()
    b0 = (torch.randint(-8, 9, (n,), generator=g).float() / 8).numpy()
    out = []
    for env in (PLAIN, d['env']):
        plan, wplan, st = build(eng, monkeypatch, d, env, U, V, b0)
        st.sp.fill_(NAN)
        st.pk.fill_(NAN)
        st.ib.b_nxt[:n].fill_(NAN)
        st.ib.epi = _lib.EPI_GRAD
        loss = torch.zeros(1, dtype=torch.float64, device='cuda')
        eng.epoch_wmrb(st, eng.adam_constants(LR), c, loss, pairs=rec.pairs)
        torch.cuda.synchronize()
        out.append(dict(sp=st.sp.clone(), pk=st.pk.clone(), D=wplan.D.clone(), delta=wplan.delta.clone(), loss=float(loss),
                        gb=st.ib.b_nxt[:n].cpu().numpy().astype(np.float64), forms=forms_of(wplan, st), blocks=wplan.user_chunks))
        if env is PLAIN:   # the fp64 sum of the weights of every item's entries: the interactions with a value > 0 and the samples
            pos = (plan.val_u > 0).cpu().numpy()
            G, A = np.zeros(n), np.zeros(n)
            for ids, w in ((plan.col_u.cpu().numpy()[pos], wplan.delta.cpu().numpy()[pos]), (wplan.R.cpu().numpy().reshape(-1), wplan.D.cpu().numpy().reshape(-1))):
                np.add.at(G, ids, w.astype(np.float64))
                np.add.at(A, ids, np.abs(w.astype(np.float64)))
    a, b = out
    what = dict(d['env'], seed=seed, kind=kind, m=m, n=n, r=r, S=S, blocks=(a['blocks'], b['blocks']), **b['forms'])
    assert not any(a['forms'].values()), a['forms']
    assert b['forms'] == expected_forms(d) and b['blocks'] == int(d['env']['TMF_USER_CHUNKS']), what
    assert seed != DYADIC_SEEDS[-1] or (b['blocks'] > 1 and d['long_lists']), what
    for k in ('sp', 'pk', 'D', 'delta'):
        assert torch.equal(a[k], b[k]), (k, what)
    assert a['loss'] == b['loss'] and np.isfinite(a['loss']) and np.abs(G).max() > 1e-3, what
    for run in (a, b):
        assert np.isfinite(run['gb']).all() and (np.abs(run['gb'] - G) <= ulp32(G) + 1e-12 * A).all(), (np.abs(run['gb'] - G).max(), what)
