"""The KernelTimer span names of every epoch - what bench.py and tools/time_*.py read - pinned as exact sets, and
_engine.run_epoch against the direct epoch_* call: same loss and same tables, bit for bit, from equal starting tables.
96 users x 64 items, r = 16, S = 8, ~600 interactions of which user 0 has 300 (a row cut into three segments at chunk = 128)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

M, N, R_, S, CHUNK, LR = 96, 64, 16, 8, 128, 0.05
MSE = {'mse_user_pass', 'mse_item_pass'}
KL = {'kl_moments', 'kl_coeffs', 'kl_user_pass', 'kl_item_pass'}
FUSED = {'wmrb_user_pass', 'wmrb_item_pass', 'wmrb_combine'}
SLICED = FUSED | {'wmrb_scores', 'wmrb_hinge', 'wmrb_gradu', 'wmrb_finish'}
BIAS = {side + name for side in ('user_', 'item_') for name in ('bias_colsum', 'bias_adam', 'adam_bias_rows')}


@pytest.fixture(scope='module')
def eng():
    from teamoflow_amd import _engine, _lib
    _lib.get()
    return _engine


@pytest.fixture(scope='module')
def prob():
    g = torch.Generator().manual_seed(11)
    u = torch.cat([torch.zeros(300, dtype=torch.int64), torch.randint(1, M, (300,), generator=g)])
    idx = torch.stack([u, torch.randint(0, N, (600,), generator=g)], 1)
    val = torch.randint(-1, 4, (600,), generator=g).float()          # both KL classes, most of them positives
    R = torch.stack([torch.randperm(N, generator=g)[:S] for _ in range(M)]).to(torch.int32)
    U0, V0 = 0.3 * torch.randn(M, R_, generator=g), 0.3 * torch.randn(N, R_, generator=g)
    return dict(idx=idx.cuda(), val=val.cuda(), R=R.cuda(), U0=U0, V0=V0)


def state(eng, prob, loss, sliced=None, biased=False):
    plan = eng.InteractionPlan(prob['idx'], prob['val'], M, N, chunk=CHUNK, csc=loss != 'wmrb')
    assert plan.seg_u.n_long >= 1 and int(plan.rowptr_u[1]) == 300    # user 0's row is cut
    wplan = None
    if loss == 'wmrb':
        wplan = eng.WmrbPlan(plan, prob['R'], chunk=CHUNK, item_slices=2 if sliced else 1, n_components=R_, sliced=sliced)
    bias = torch.zeros(R_) if biased else None
    return eng.TrainState(prob['U0'], prob['V0'], plan, R_, wplan, kl=loss == 'kl', user_bias=bias, item_bias=bias)


def run(eng, st, call):
    """call(st, adam, loss_out, prof) -> (span names, loss, the tables and gradient tables the epoch wrote)."""
    prof, loss = eng.KernelTimer(), torch.zeros(1, dtype=torch.float64, device='cuda')
    call(st, eng.adam_constants(LR), loss, prof)
    torch.cuda.synchronize()
    assert all(b is not None for spans in prof.spans.values() for _, b in spans)     # every bracket was closed
    tables = [t.clone() for t in (st.U, st.V, st.U_nxt, st.V_nxt) if t is not None]
    tables += [t.clone() for side in (st.bias_u, st.bias_v) if side is not None for t in (side.G, side.W, side.b)]
    return set(prof.spans), loss.clone(), tables


def same(a, b):
    return a[0] == b[0] and torch.equal(a[1], b[1]) and len(a[2]) == len(b[2]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


@pytest.mark.parametrize('loss,sliced,names', [('mse', None, MSE), ('kl', None, KL), ('wmrb', False, FUSED), ('wmrb', True, SLICED)],
                         ids=['mse', 'kl', 'wmrb_fused', 'wmrb_sliced'])
def test_span_names_and_run_epoch(eng, prob, monkeypatch, loss, sliced, names):
    for name in ('TMF_ROW_STATIONARY', 'TMF_SCORES5', 'TMF_SCORES6', 'TMF_ROWS4'):
        monkeypatch.delenv(name, raising=False)
    c = N / S
    direct = {'mse': lambda st, adam, out, prof: eng.epoch_mse(st, adam, out, prof=prof),
              'kl': lambda st, adam, out, prof: eng.epoch_kl(st, adam, out, prof=prof),
              'wmrb': lambda st, adam, out, prof: eng.epoch_wmrb(st, adam, c, out, prof=prof)}[loss]
    a = run(eng, state(eng, prob, loss, sliced), direct)
    b = run(eng, state(eng, prob, loss, sliced), lambda st, adam, out, prof: eng.run_epoch(st, adam, out, loss, c, prof=prof))
    assert a[0] == names and b[0] == names
    assert float(a[1]) > 0 and same(a, b)


def test_span_names_of_a_biased_epoch(eng, prob):
    from teamoflow_amd import _lib
    grad = dict(item_epi=_lib.EPI_GRAD, user_epi=_lib.EPI_GRAD)
    a = run(eng, state(eng, prob, 'mse', biased=True), lambda st, adam, out, prof: eng.epoch_biased(st, adam, out, 'mse', prof=prof))
    assert a[0] == MSE | BIAS
    # the passes inside: run_epoch and epoch_mse write the same loss and gradient tables as epoch_biased read them from
    b = run(eng, state(eng, prob, 'mse', biased=True), lambda st, adam, out, prof: eng.epoch_mse(
        st, adam, out, item_out=st.bias_v.G, user_out=st.bias_u.G, prof=prof, **grad))
    d = run(eng, state(eng, prob, 'mse', biased=True), lambda st, adam, out, prof: eng.run_epoch(
        st, adam, out, 'mse', item_out=st.bias_v.G, user_out=st.bias_u.G, prof=prof, **grad))
    assert b[0] == d[0] == MSE and same(b, d)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2][2], b[2][2]) and torch.equal(a[2][5], b[2][5])   # loss, user G, item G
