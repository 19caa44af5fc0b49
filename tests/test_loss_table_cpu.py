"""The table of loss records (_engine.LOSSES) behind every dispatch on a loss: the module-level tuples derived from it against their
values typed out, loss_name and its TypeError, every record's parameter, denominator and work term against the expressions
_fit_sparse used to spell out per name, the facts of the table family, and the table DESIGN.md prints.  No GPU, no libtmf.so."""
import os
import types

import pytest

from teamoflow_amd import _engine
from teamoflow_amd.mf import loss_graphs as LG
from teamoflow_amd.mf import matrix_factorization as M

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
NAMES = ('mse', 'wmrb', 'kl', 'logistic', 'logistic_w', 'bpr', 'warp', 'warp_kos', 'softmax', 'full_softmax')
GRAPHS = {'mse': LG.MSELoss(), 'wmrb': LG.WMRBLoss(), 'kl': LG.KLDivergenceLoss(), 'logistic': LG.LogisticLoss(),
          'logistic_w': LG.LogisticLoss(weighted=True), 'bpr': LG.BPRLoss(), 'warp': LG.WARPLoss(), 'warp_kos': LG.KOSWARPLoss(k=3, n=4),
          'softmax': LG.SampledSoftmaxLoss(), 'full_softmax': LG.FullSoftmaxLoss()}
NOT_A_LOSS = ('{} is not a loss the HIP engine trains (MSELoss, WMRBLoss, KLDivergenceLoss, LogisticLoss, BPRLoss, WARPLoss, KOSWARPLoss, '
              'SampledSoftmaxLoss, FullSoftmaxLoss)')


def test_the_derived_tuples_are_the_literals_they_replaced():
    assert _engine.LOGISTIC_LOSSES == ('logistic', 'logistic_w')
    assert _engine.SLICED_ONLY == ('bpr', 'warp', 'warp_kos', 'softmax')
    assert _engine.PAIR_LOSSES == ('wmrb', 'bpr', 'warp', 'warp_kos', 'softmax')
    assert M.ENGINE_LOSSES == (LG.MSELoss, LG.WMRBLoss, LG.KLDivergenceLoss, LG.LogisticLoss, LG.BPRLoss, LG.WARPLoss, LG.KOSWARPLoss,
                               LG.SampledSoftmaxLoss, LG.FullSoftmaxLoss)
    assert M.TABLE_LOSSES == (LG.WMRBLoss, LG.BPRLoss, LG.WARPLoss, LG.KOSWARPLoss, LG.SampledSoftmaxLoss)
    assert M.PAIR_STEP_LOSSES == (LG.BPRLoss, LG.WARPLoss, LG.KOSWARPLoss, LG.SampledSoftmaxLoss)
    assert M.PAIR_ROW_LOSSES == (LG.BPRLoss, LG.WARPLoss, LG.KOSWARPLoss, LG.SampledSoftmaxLoss, LG.FullSoftmaxLoss)


def test_loss_name_of_every_class_and_of_nothing_else():
    assert [_engine.loss_name(graph) for graph in GRAPHS.values()] == list(NAMES)
    assert _engine.loss_name(LG.LogisticLoss(weighted=False)) == 'logistic'
    assert _engine.loss_name(LG.SampledSoftmaxLoss(True)) == 'softmax'
    strangers = [type('My' + type(graph).__name__, (type(graph),), {})() for graph in GRAPHS.values()] + [object(), 'mse', None]
    for bad in strangers:   # a subclass of each class (LogisticLoss twice: its subclass is a stranger whatever its weighted) and non-losses
        with pytest.raises(TypeError) as err:
            _engine.loss_name(bad)
        assert str(err.value) == NOT_A_LOSS.format(type(bad).__name__)


def test_the_table_has_the_ten_names_in_order():
    assert tuple(_engine.LOSSES) == NAMES and all(rec.name == name for name, rec in _engine.LOSSES.items())
    assert all(rec.cls is type(GRAPHS[name]) and rec.prose for name, rec in _engine.LOSSES.items())
    assert [rec.weighted for rec in _engine.LOSSES.values()] == [None, None, None, False, True, None, None, None, None, None]
    assert {name: rec.family for name, rec in _engine.LOSSES.items()} == dict(
        mse='list', kl='list', logistic='list', logistic_w='list', wmrb='table', bpr='table', warp='table', warp_kos='table',
        softmax='table', full_softmax='catalog')
    assert {name: rec.epoch for name, rec in _engine.LOSSES.items()} == dict(
        mse=_engine.epoch_mse, kl=_engine.epoch_kl, logistic=_engine.epoch_logistic, logistic_w=_engine.epoch_logistic,
        wmrb=_engine.epoch_wmrb, bpr=_engine.epoch_wmrb, warp=_engine.epoch_wmrb, warp_kos=_engine.epoch_wmrb, softmax=_engine.epoch_wmrb,
        full_softmax=_engine.epoch_full_softmax)
    assert {name: rec.route for name, rec in _engine.LOSSES.items() if rec.route} == dict(
        kl='kl', logistic='logistic', logistic_w='logistic', bpr='pair', warp='pair', warp_kos='pair', softmax='pair', full_softmax='pair')
    assert {name: rec.flag for name, rec in _engine.LOSSES.items() if rec.flag} == dict(kl='kl', full_softmax='full_softmax')
    assert {name: rec.feeds for name, rec in _engine.LOSSES.items() if rec.feeds != 'dense'} == dict(
        kl='serial', wmrb='samples', bpr='samples', warp='samples', warp_kos='samples', softmax='samples')


@pytest.mark.parametrize('catalog_scale', [False, True])
def test_the_parameter_of_every_loss(catalog_scale):
    """n_items = 7, n_samples = 2: the ratio is 3.5 by true division of the constructor's ints."""
    want = dict.fromkeys(NAMES, 0.0)
    want.update(wmrb=3.5, softmax=3.5 if catalog_scale else 1.0, warp_kos=(3, 4))
    for name, rec in _engine.LOSSES.items():
        graph = LG.SampledSoftmaxLoss(catalog_scale) if name == 'softmax' else GRAPHS[name]
        model = M.MatrixFactorization(4, loss_graph=graph, n_users=5, n_items=7, n_samples=2)
        got = rec.param(model)
        assert got == want[name] and type(got) is type(want[name]), name


def test_the_denominator_and_the_work_term_of_every_loss():
    """Against the expressions _fit_sparse spelled out per name before the table."""
    plan = types.SimpleNamespace(nnz=1000, n_pos=600, n_users=30, n_items=70)
    wplan = types.SimpleNamespace(S=8)
    pair_losses = ('wmrb', 'bpr', 'warp', 'warp_kos', 'softmax')
    for loss, rec in _engine.LOSSES.items():
        denom = plan.n_pos if loss in pair_losses + ('full_softmax',) else 1 if loss == 'kl' else plan.nnz
        work = plan.nnz + (plan.n_users * wplan.S if loss in pair_losses else 0) + (plan.n_users * plan.n_items if loss == 'full_softmax' else 0)
        assert rec.denominator(plan) == denom and rec.work(plan, None if loss not in pair_losses else wplan) == work, loss
        form = rec.plan_form()
        assert form == dict(user_chunks=1 if loss in pair_losses else _engine.mse_user_chunks(), csc=loss not in pair_losses), loss


def test_the_table_family():
    table = {name: rec for name, rec in _engine.LOSSES.items() if rec.table}
    assert tuple(table) == _engine.PAIR_LOSSES and all(callable(rec.pair_step) for rec in table.values())
    assert all(rec.pair_step is None and not rec.sliced_only and not rec.ranked and not rec.plan_needs
               for name, rec in _engine.LOSSES.items() if name not in table)
    assert [name for name, rec in table.items() if not rec.sliced_only] == ['wmrb']
    assert [name for name, rec in table.items() if rec.ranked] == ['warp', 'warp_kos']
    assert {name: rec.plan_needs for name, rec in table.items() if rec.plan_needs} == dict(warp_kos=('kos_omega',))
    assert list(_engine.PAIRS) == ['hinge', 'bpr', 'warp', 'warp_kos', 'softmax']
    assert [rec.name for rec in _engine.PAIRS.values()] == list(_engine.PAIR_LOSSES)
    assert len({rec.pair_step for rec in table.values()}) == 5


def test_prepare_builds_what_the_record_names_and_the_plan_remembers_it():
    """Loss.prepare on a real WmrbPlan (CPU tensors): what it builds, and WmrbPlan.prepared - the list TrainState.set_negatives replays
    on the next plan - whoever built it: the record's hook, a caller by hand, or the first epoch."""
    import torch
    g = torch.Generator().manual_seed(3)
    idx = torch.stack([torch.arange(12).repeat_interleave(3), torch.randint(0, 9, (36,), generator=g)], 1)
    plan = _engine.InteractionPlan(idx, torch.ones(36), 12, 9, csc=False)
    R = torch.stack([torch.randperm(9, generator=g)[:4] for _ in range(12)]).to(torch.int32)
    for name, built in (('wmrb', []), ('bpr', []), ('softmax', []), ('warp', [('sample_rank', ())]),
                        ('warp_kos', [('sample_rank', ()), ('kos_omega', (plan.nnz,))])):
        wplan = _engine.WmrbPlan(plan, R, item_slices=2, n_components=4, sliced=True)
        assert wplan.prepared == []
        _engine.LOSSES[name].prepare(wplan, plan)
        _engine.LOSSES[name].prepare(wplan, plan)   # what is there is built, and noted, once
        assert wplan.prepared == built, name
        assert (getattr(wplan, '_rank', None) is not None) == (name in ('warp', 'warp_kos')), name
        assert (getattr(wplan, 'omega', None) is not None) == (name == 'warp_kos'), name
    by_hand = _engine.WmrbPlan(plan, R, item_slices=2, n_components=4, sliced=True)
    by_hand.sample_rank()
    assert by_hand.prepared == [('sample_rank', ())]


def test_the_hinge_and_the_global_moments():
    assert [name for name, rec in _engine.LOSSES.items() if rec.hinge] == ['wmrb']
    assert [name for name, rec in _engine.LOSSES.items() if rec.global_moments] == ['kl']
    assert {name: rec.pairs for name, rec in _engine.LOSSES.items() if rec.pairs} == dict(
        wmrb='hinge', bpr='bpr', warp='warp', warp_kos='warp_kos', softmax='softmax')


def test_the_refusals_of_run_epoch_and_epoch_wmrb_keep_their_texts():
    class State:
        wplan = types.SimpleNamespace(sliced=False)
        plan = r = None
    for loss in _engine.SLICED_ONLY:
        with pytest.raises(ValueError) as err:
            _engine.run_epoch(State(), None, None, loss)
        assert str(err.value) == f"run_epoch: unknown loss '{loss}' on a state without a sliced WmrbPlan"
        with pytest.raises(ValueError) as err:
            _engine.epoch_wmrb(State(), None, 0.0, None, pairs=loss)
        assert str(err.value) == f'epoch_wmrb: pairs={loss} needs the sliced user pass (wmrb_plan_for(force_sliced=True))'
    with pytest.raises(ValueError) as err:
        _engine.run_epoch(State(), None, None, 'full_softmax')
    assert str(err.value) == "run_epoch: unknown loss 'full_softmax' on a state built without full_softmax=True"
    with pytest.raises(ValueError) as err:
        _engine.run_epoch(State(), None, None, 'hinge')
    assert str(err.value) == "run_epoch: unknown loss 'hinge'"
    with pytest.raises(ValueError) as err:
        _engine.epoch_wmrb(State(), None, 0.0, None, pairs='wmrb')
    assert str(err.value) == "epoch_wmrb: pairs='wmrb' (hinge, bpr, warp, warp_kos or softmax)"
    model = types.SimpleNamespace(optimizer='fresh_adam', loss_graph=LG.KLDivergenceLoss())
    with pytest.raises(ValueError) as err:
        _engine.form_loss(model, 'mini-batch', 'unused')
    assert str(err.value) == 'KLDivergenceLoss has no mini-batch form (its moments are global)'
    assert [_engine.form_loss(types.SimpleNamespace(loss_graph=graph), 'multi-GPU', 'unused') for name, graph in GRAPHS.items()
            if name != 'kl'] == [name for name in NAMES if name != 'kl']


def design_rows():
    head = ['name', 'class', 'family', 'sliced only', 'pair step or epoch', 'parameter', 'denominator', 'route row']
    rows = [head, ['---'] * len(head)]
    for rec in _engine.LOSSES.values():
        cls = rec.kind + ('' if rec.weighted is None else f'(weighted={rec.weighted})')
        rows.append([f'`{rec.name}`', f'`{cls}`', rec.family, ('yes' if rec.sliced_only else 'no') if rec.table else '-',
                     f'`{(rec.pair_step or rec.epoch).__name__}`', f'`{rec.param.__name__}`', rec.denom, f'`{rec.route}`' if rec.route else '-'])
    return rows


def test_design_md_prints_the_loss_table():
    with open(os.path.join(ROOT, 'DESIGN.md')) as f:
        design = f.read()
    printed = '\n'.join('| ' + ' | '.join(cells) + ' |' for cells in design_rows())
    printed += '\n\n' + '\n'.join(f'- `{rec.name}`: {rec.prose}' for rec in _engine.LOSSES.values())
    assert '\n\n' + printed + '\n\n' in design, 'DESIGN.md, "What a loss is made of", should print:\n' + printed
    assert design.index('### What trains where') < design.index('### What a loss is made of') < design.index(printed)
