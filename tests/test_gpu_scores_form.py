"""The one stream plan a state builds (_engine.scores_form -> TrainState._adopt_wplan) and the launch each plan class makes of its
own kernel: each of the four scores kernels forced by its switch, and TMF_SCORES5=1 with TMF_SCORES7=1, at the smallest shape that
crosses the group borders - 300 users (past the 256-user groups of scores5 / scores7 and the 64-user groups of scores6), 2000 items
in 2 slices, r = 128 fp32 (the one width all four kernels exist for), S = 50, 5000 interactions."""
import pytest
import torch

from test_fuzz_draws_cpu import FORM_KEYS
from test_gpu_scores5 import problem

pytestmark = pytest.mark.gpu

M, N, R_, S, NNZ = 300, 2000, 128, 50, 5000
FORMS = {   # switches -> the slot that is filled (None: scores3)
    'scores3': (dict(TMF_SCORES5='0', TMF_SCORES6='0', TMF_SCORES7='0'), None),
    'scores5': (dict(TMF_SCORES5='1'), 's5'),
    'scores6': (dict(TMF_SCORES6='1'), 's6'),
    'scores7': (dict(TMF_SCORES7='1'), 's7'),
    'scores5+scores7': (dict(TMF_SCORES5='1', TMF_SCORES7='1'), 's7'),
}


@pytest.fixture(scope='module')
def eng():
    from teamoflow_amd import _engine, _lib
    _lib.get()
    return _engine


def slots(wplan):
    return [name for name in ('s5', 's6', 's7') if getattr(wplan, name) is not None]


def run(eng, monkeypatch, form, data):
    idx, val, R, U, V = data
    for k in FORM_KEYS:
        monkeypatch.delenv(k, raising=False)
    switches, slot = FORMS[form]
    for k, v in dict(switches, TMF_FORCE_SLICED='1', TMF_ITEM_SLICES='2').items():
        monkeypatch.setenv(k, v)
    plan = eng.InteractionPlan(idx, val, M, N)
    wplan = eng.wmrb_plan_for(plan, R, R_)
    st = eng.TrainState(U, V, plan, R_, wplan)
    assert wplan.sliced and wplan.n_slices == 2 and slots(wplan) == ([slot] if slot else []), form
    assert eng.scores_form_of(plan, wplan, R_) == ((form.split('+')[-1], True) if slot else ('scores3', False))
    st.sp.fill_(float('nan'))
    st.pk.fill_(float('nan'))
    loss = torch.zeros(1, dtype=torch.float64, device='cuda')
    eng.epoch_wmrb(st, eng.adam_constants(0.05), N / S, loss)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(st.sp).all()) and bool(torch.isfinite(st.pk).all()), form   # every score was written
    out = dict(sp=st.sp.clone(), pk=st.pk.clone(), D=wplan.D.clone(), delta=wplan.delta.clone(), loss=float(loss),
               U=st.U_nxt.clone(), V=st.V_nxt.clone())
    # another table of the same shape: the state re-plans and fills the same single slot
    st.set_negatives(torch.roll(R, 1, 0))
    assert st.wplan is not wplan and slots(st.wplan) == ([slot] if slot else []), form
    return out


@pytest.fixture(scope='module')
def tables():
    """(dyadic, Gaussian) problems of the shape, built once; nothing writes them."""
    return problem(M, N, R_, S, NNZ, seed=4, dyadic=True), problem(M, N, R_, S, NNZ, seed=4)


@pytest.fixture(scope='module')
def reference(eng, tables):
    """The scores3 runs the stream forms are compared to, computed once."""
    mp = pytest.MonkeyPatch()
    try:
        return [run(eng, mp, 'scores3', data) for data in tables]
    finally:
        mp.undo()


@pytest.mark.parametrize('form', [f for f in FORMS if f != 'scores3'])
def test_a_forced_form_fills_its_one_slot_and_equals_scores3(eng, monkeypatch, tables, reference, form):
    """Only the scores kernel differs from the scores3 run - same scores order, same pair step, same list entries.  On dyadic tables
    (every dot product exact whatever its summation tree: the generator tests/test_gpu_scores5/6/7 prove the forms bit-identical
    with) sp, pk, D, delta, the loss and both stepped tables are bit-equal.  On Gaussian tables the kernels differ in the order of
    the fp32 sum inside a dot product, so sp and pk are held to the closeness bound of those tests, 2e-6 of the largest score, and
    the loss to 1e-6."""
    a, b = reference[0], run(eng, monkeypatch, form, tables[0])
    for k in ('sp', 'pk', 'D', 'delta', 'U', 'V'):
        assert torch.equal(a[k], b[k]), (form, k)
    assert a['loss'] == b['loss']
    a, b = reference[1], run(eng, monkeypatch, form, tables[1])
    scale = float(a['sp'].abs().max())
    assert float((a['sp'] - b['sp']).abs().max()) <= 2e-6 * scale and float((a['pk'] - b['pk']).abs().max()) <= 2e-6 * scale
    assert abs(a['loss'] - b['loss']) <= 1e-6 * abs(a['loss'])
