"""Which kernel forms a WMRB fit takes (_engine.scores_form over _engine.SCORES_FORMS, row_stationary_wanted, rows4_wanted,
choose_wmrb_user_pass), replayed against the record of the commit before the table existed (tests/golden/kernel_forms.json); the
table DESIGN.md prints; the shape assertions of the selection functions; and the one declaration of the environment switches
(_engine.SWITCHES).  Needs libtmf.so's host queries, no GPU."""
import collections
import importlib.util
import json
import os
import re
import string

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
spec = importlib.util.spec_from_file_location('make_golden', os.path.join(GOLDEN, 'make_golden.py'))
make_golden = importlib.util.module_from_spec(spec)
spec.loader.exec_module(make_golden)

F32, BF16 = torch.float32, torch.bfloat16
C4 = (1_000_000, 100_000, 1024, 100_000_000)      # n_users, n_items, n_samples, nnz
C5 = (156_250, 1_000_000, 1024, 15_600_000)       # the config-5 shard
MID = (100_000, 20_000, 256, 5_000_000)


@pytest.fixture
def eng(monkeypatch):
    from teamoflow_amd import _engine
    for k in [k for k in os.environ if k.startswith('TMF_') and k != 'TMF_LIB']:
        monkeypatch.delenv(k)
    monkeypatch.setenv('TMF_SLAB_BUDGET', str(64 << 30))   # rows4_wanted would read the card's memory
    return _engine


def test_every_recorded_kernel_form_is_todays():
    with open(os.path.join(GOLDEN, 'kernel_forms.json')) as f:
        doc = json.load(f)
    # the record is of this grid ...
    assert {k: tuple(v) for k, v in doc['shapes'].items()} == make_golden.FORM_SHAPES
    assert [tuple(w) for w in doc['widths']] == list(make_golden.FORM_WIDTHS) and doc['slab_budget'] == make_golden.FORM_SLAB_BUDGET
    assert [tuple(tuple(kv) for kv in s) for s in doc['settings']] == list(make_golden.FORM_SETTINGS)
    recorded = [(doc['outcomes'][string.ascii_letters.index(ch)], ns) for ch, ns in zip(doc['rows'], doc['n_slices'], strict=True)]
    assert len(recorded) == len(make_golden.FORM_SHAPES) * len(make_golden.FORM_WIDTHS) * len(make_golden.FORM_SETTINGS) == 896
    # ... and it reaches every form and both values of every flag
    forms = collections.Counter(text.split()[0] for text, _ in recorded)
    assert set(forms) == {'scores3', 'scores5', 'scores6', 'scores7'} and min(forms.values()) >= 20, forms
    for flag in ('forced', 'row_stationary', 'rows4', 'sliced'):
        assert 0 < sum(flag in text.split() for text, _ in recorded) < len(recorded), flag
    got = make_golden.kernel_form_outcomes()
    wrong = [(i, want, have) for i, (want, have) in enumerate(zip(recorded, got, strict=True)) if want != have]
    assert not wrong, f'{len(wrong)} of {len(got)} rows differ, first (row, recorded, now) = {wrong[0]}'


def test_design_md_prints_the_scores_form_table(eng):
    with open(os.path.join(ROOT, 'DESIGN.md')) as f:
        design = f.read()
    rows = [['form', 'switch', 'library query', 'plan class', 'slot'], ['---'] * 5]
    rows += [[f'`{f.name}`', f'`{f.switch}`', f'`{f.supported}`', f'`{f.plan.__name__}`', f'`WmrbPlan.{f.slot}`'] for f in eng.SCORES_FORMS]
    printed = '\n'.join('| ' + ' | '.join(cells) + ' |' for cells in rows)
    assert '\n\n' + printed + '\n\n' in design, 'DESIGN.md, "Which scores kernel runs", should print:\n' + printed
    assert [f.name for f in eng.SCORES_FORMS] == ['scores7', 'scores6', 'scores5']   # the precedence


def test_scores7_selection(eng, monkeypatch):
    """Default: on at C4 (a group of 256 users meets every row of a slice 2.9 times), off at the config-5 shard (0.29: scores6
    stays), off at the mid shape and every small shape; TMF_SCORES7 forces it where the kernel exists; TMF_SCORES5 / TMF_SCORES6 = 1
    win over the default; the other choices answer as before."""
    form = eng.scores_form
    assert form(*C4, 128, F32) == ('scores7', False)
    assert form(*C5, 256, BF16) == ('scores6', False)
    assert form(*C5, 128, F32) == ('scores6', False)                   # fp32 rows there too: 0.29 entries per row of a group
    assert form(*MID, 128, F32) == ('scores3', False)
    for r, dtype in ((128, BF16), (64, F32), (256, F32)):              # no scores7 kernel: scores6's own rule says no at C4
        assert form(*C4, r, dtype) == ('scores3', False)
    assert form(*C4, 128, F32, sliced=False) == form(*C4, 128, F32, on_gpu=False) == ('scores3', False)
    monkeypatch.setenv('TMF_SCORES5', '1')
    assert form(*C4, 128, F32) == ('scores5', True) and form(*C4, 128, F32, item_lists=False) == ('scores3', False)
    monkeypatch.delenv('TMF_SCORES5')
    monkeypatch.setenv('TMF_SCORES6', '1')
    assert form(*C4, 128, F32) == ('scores6', True)
    monkeypatch.delenv('TMF_SCORES6')
    monkeypatch.setenv('TMF_SCORES7', '0')
    assert form(*C4, 128, F32) == ('scores3', False)                   # and scores6's own rule says no at C4
    assert form(*C5, 256, BF16) == ('scores6', False)
    monkeypatch.setenv('TMF_SCORES7', '1')
    assert form(*MID, 128, F32) == form(*C5, 128, F32) == ('scores7', True)
    assert form(*MID, 128, BF16) == form(*MID, 200, F32) == ('scores3', False)
    assert form(3_000_000, 100_000, 1024, 1000, 128, F32) == ('scores3', False)   # m S >= 2^31: int32 places
    # the rows behind one whose streams did not fit
    monkeypatch.delenv('TMF_SCORES7')
    assert form(*C4, 128, F32, after='scores7') == ('scores3', False)
    assert form(*C5, 256, BF16, after='scores7') == ('scores6', False) and form(*C5, 256, BF16, after='scores6') == ('scores3', False)


def test_the_item_pass_form_follows_the_shape(eng, monkeypatch):
    """Row-stationary exactly where the slab form cannot block the users for the L2s (its slab would exceed the budget at ~4 MB
    blocks): the config-5 shard, not C4 and not the small shapes.  TMF_ROWS4 = 0 | 1 forces either."""
    assert eng.rows4_wanted(256, BF16, n_users=1_250_000, n_items=1_000_000)          # one GPU's share of config 5
    assert not eng.rows4_wanted(128, F32, n_users=1_000_000, n_items=100_000)         # C4: 163 blocks, 8.3 GB of slab
    assert not eng.rows4_wanted(64, F32, n_users=6040, n_items=3706)                  # C3
    assert not eng.rows4_wanted(8, F32, n_users=10_000_000, n_items=10_000_000)       # rows of fewer than 16 lanes: no such kernel
    monkeypatch.setenv('TMF_ROWS4', '1')
    assert eng.rows4_wanted(128, F32, n_users=1000, n_items=1000)
    monkeypatch.setenv('TMF_ROWS4', '0')
    assert not eng.rows4_wanted(256, BF16, n_users=1_250_000, n_items=1_000_000)
    assert eng.rows5_user_chunks(1_250_000, 256, BF16) == 153      # 4 MB of bf16 rows per block


def test_the_user_pass_forms_follow_the_shape_too(eng, monkeypatch):
    """Short (user, 4 MB slice) visits - the config-5 shard: 9 rows - take the flat-stream scores kernel and the row-stationary
    gradU with 3.2 MB slices; C4 (88 rows per visit) and the small configurations keep scores3 / gradu3."""
    assert eng.short_visits(1_250_000, 1_000_000, 1024, 125_000_000, 256, BF16)
    assert not eng.short_visits(1_000_000, 100_000, 1024, 100_000_000, 128, F32)
    assert not eng.short_visits(6040, 3706, 1853, 1_000_209, 64, F32) and not eng.short_visits(50, 100, 5, 200, 128, F32)
    assert eng.row_stationary_wanted(1_250_000, 1_000_000, 1024, 125_000_000, 256, BF16)
    assert not eng.row_stationary_wanted(1_000_000, 100_000, 1024, 100_000_000, 128, F32)
    monkeypatch.setenv('TMF_ROW_STATIONARY', '0')
    assert not eng.row_stationary_wanted(1_250_000, 1_000_000, 1024, 125_000_000, 256, BF16)


OLD_FORM_KEYS = ('TMF_ROWS4', 'TMF_ROWS5', 'TMF_ROWS5_TARGET', 'TMF_SCORES5', 'TMF_SCORES6', 'TMF_S6_SLICE_BYTES', 'TMF_SCORES7',
                 'TMF_S7_SLICE_BYTES', 'TMF_S7_SLOTS', 'TMF_S7_FILL', 'TMF_ROW_STATIONARY', 'TMF_ITEM_SLICES', 'TMF_USER_CHUNKS',
                 'TMF_FORCE_SLICED', 'TMF_SLICE_XCD', 'TMF_G4_USERS', 'TMF_ROWS4_PER_LAUNCH')


def test_the_switches_are_declared_once(eng):
    from test_fuzz_draws_cpu import FORM_KEYS
    assert set(OLD_FORM_KEYS) <= set(FORM_KEYS) == {k for k, (_, form) in eng.SWITCHES.items() if form}
    assert {'TMF_FORCE_FUSED', 'TMF_S7_BUILD', 'TMF_HINGE_ORDER', 'TMF_S5_PACE', 'TMF_S5_LAG'} <= set(FORM_KEYS)   # what the tuple missed
    assert all(isinstance(text, str) and text and isinstance(form, bool) for text, form in eng.SWITCHES.values())
    with open(eng.__file__) as f:
        source = f.read()
    assert source.count('os.environ') == 1 and re.search(r'def switch\(name, default=None\):\n(?:    .*\n)+?    return os\.environ\.get', source)
    assert set(re.findall(r"switch\('(TMF_[A-Z0-9_]+)'", source)) <= set(eng.SWITCHES)
    with pytest.raises(KeyError, match='TMF_NOT_A_SWITCH is not declared'):
        eng.switch('TMF_NOT_A_SWITCH')
    with open(os.path.join(ROOT, 'README.md')) as f:
        readme = f.read()
    tunables = readme[readme.index('Tunables (environment, all optional)'):].split('\n\n')[0]
    assert not [k for k in eng.SWITCHES if f'`{k}`' not in tunables and f'`{k}=' not in tunables]
