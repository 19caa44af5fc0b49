"""_engine.Scores7Plan (the streams tmf_wmrb_scores7 walks: include/tmf.h), built on CPU tensors, against a NumPy brute force:
every (user, item) pair the epoch needs sits in exactly one non-pad slot; the users of a step share its item and its chunk; place[]
restricted to a chunk is a bijection onto the chunk's sp / p addresses; the slots of a user are consecutive and ascending; a
sub-chunk holds at most `slots` entries."""
import numpy as np
import pytest
import torch


def _lib_and_engine():
    import __graft_entry__ as ge
    from teamoflow_amd import _engine as E, _lib
    ge.build()
    return _lib.load_library(), E


def _problem(m, n, S, nnz, seed, empty_user=None):
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0, m, (nnz,), generator=g)
    j = torch.randint(0, n, (nnz,), generator=g)
    if empty_user is not None and m > 1:
        u[u == empty_user] = (empty_user + 1) % m
    key = torch.unique(u * n + j)
    idx = torch.stack([key // n, key % n], 1)
    val = torch.randint(-1, 6, (key.numel(),), generator=g).float()
    R = torch.stack([torch.randperm(n, generator=g)[:S] for _ in range(m)]).to(torch.int32)
    return idx, val, R


def _check(E, lib, m, n, S, nnz, seed, slice_rows, slots=None, empty_user=None):
    return check_streams(E, lib, m, n, S, _problem(m, n, S, nnz, seed, empty_user), slice_bytes=slice_rows * 512, slots=slots,
                         empty_user=empty_user)


def check_streams(E, lib, m, n, S, problem, r=128, slice_bytes=None, slots=None, empty_user=None, item_slices=2):
    """The brute-force invariants of the module's docstring for the Scores7Plan of ``problem`` = (idx [nnz, 2], val [nnz],
    R [m, S]) as CPU tensors - any problem: COO pairs in any order, ids repeated inside a row of R, positives among the negatives."""
    K = E.Scores7Plan.K
    UG, cap = lib.tmf_wmrb_scores7_users_per_group(), lib.tmf_wmrb_scores7_slots()
    idx, val, R = problem
    plan = E.InteractionPlan(idx, val, m, n)
    wplan = E.WmrbPlan(plan, R, item_slices=item_slices, n_components=r, sliced=True)
    s7 = E.Scores7Plan(plan, wplan, r, torch.float32, slice_bytes=slice_bytes, slots=slots)
    SL = slots or cap
    assert s7.slots == SL and s7.pad_slot == cap and s7.users_per_group == UG and K == 4
    ng, ns, width = s7.n_groups, s7.n_slices, s7.width
    assert ng == -(-m // UG) and ns == -(-n // width) and s7.n_entries == plan.nnz + m * S
    steps = s7.steps.numpy().view(np.uint32)
    place = s7.place.numpy()
    sub_step, sub_place, chunk_sub = s7.sub_step.numpy(), s7.sub_place.numpy(), s7.chunk_sub.numpy()
    assert chunk_sub.shape == (ns * ng + 1,) and chunk_sub[0] == 0 and (np.diff(chunk_sub) >= 0).all()
    n_sub = int(chunk_sub[-1])
    assert sub_step.shape == sub_place.shape == (n_sub + 1,) and sub_step[-1] == s7.n_steps and sub_place[-1] == s7.n_entries
    assert steps.shape == (s7.n_steps + 1, 4) and place.shape == (s7.n_entries,)
    assert (np.diff(sub_place) <= SL).all() and (np.diff(sub_place) > 0).all()
    Rs, user_of, col, rowptr = wplan.R.numpy(), plan.user_of.numpy(), plan.col_u.numpy(), plan.rowptr_u.numpy()
    if empty_user is not None and m > 1:
        assert rowptr[empty_user] == rowptr[empty_user + 1]
    seen_sp, seen_p = np.zeros(m * S, dtype=np.int32), np.zeros(max(plan.nnz, 1), dtype=np.int32)
    assert (np.repeat(np.arange(m), np.diff(rowptr)) == user_of).all()     # the CSR's two views of an interaction's user agree
    # the chunk of every place by brute force: negative (u, s) -> place u * S + s, interaction k -> place ~k
    all_places = np.concatenate([np.arange(m * S, dtype=np.int64), ~np.arange(plan.nnz, dtype=np.int64)])
    all_chunks = np.concatenate([((Rs.astype(np.int64) // width) * ng + (np.arange(m, dtype=np.int64) // UG)[:, None]).reshape(-1),
                                 (col.astype(np.int64) // width) * ng + user_of.astype(np.int64) // UG])
    by_chunk = np.argsort(all_chunks, kind='stable')
    chunk_edge = np.searchsorted(all_chunks[by_chunk], np.arange(ns * ng + 1))
    for c in range(ns * ng):
        sl, grp = divmod(c, ng)
        want = set(all_places[by_chunk[chunk_edge[c]:chunk_edge[c + 1]]].tolist())
        got = set()
        for sub in range(chunk_sub[c], chunk_sub[c + 1]):
            pl = place[sub_place[sub]:sub_place[sub + 1]]
            slot_user = np.where(pl >= 0, pl // S, user_of[np.where(pl < 0, ~pl, 0)])
            assert (np.diff(slot_user) >= 0).all()                      # slots are numbered by user ...
            for u in np.unique(slot_user):                              # ... and a user's slots are consecutive addresses: first p, then sp
                mine = pl[slot_user == u]
                neg, pos = mine[mine >= 0], ~mine[mine < 0]
                assert (mine[:len(pos)] < 0).all() and (np.diff(neg) > 0).all() and (np.diff(pos) > 0).all()
            filled = np.zeros(len(pl), dtype=np.int32)
            prev = (-1, -1)
            for st in steps[sub_step[sub]:sub_step[sub + 1]]:
                item = int(st[0])
                users = [(int(st[1]) >> (8 * k)) & 0xff for k in range(K)]
                slots4 = [(int(st[2 + k // 2]) >> (16 * (k % 2))) & 0xffff for k in range(K)]
                assert item // width == sl and item < n
                real = [k for k in range(K) if slots4[k] != cap]
                assert real and real == list(range(len(real)))          # pads sit behind the step's entries
                assert all(grp * UG + lu < m for lu in users)           # pads name a resident row too
                keys = [(item, users[k]) for k in real]
                assert keys == sorted(keys) and keys[0] >= prev         # by (item, local user) through the sub-chunk
                prev = keys[-1]
                for k in real:
                    assert slots4[k] < len(pl)
                    filled[slots4[k]] += 1
                    where, u = int(pl[slots4[k]]), grp * UG + users[k]
                    if where >= 0:
                        assert where // S == u and Rs[u, where % S] == item
                    else:
                        assert user_of[~where] == u and col[~where] == item
            assert (filled == 1).all()                                   # every slot of the sub-chunk is written exactly once
            got_sub = set(int(x) for x in pl)
            assert len(got_sub) == len(pl) and not (got & got_sub)
            got |= got_sub
            np.add.at(seen_sp, pl[pl >= 0], 1)
            np.add.at(seen_p, ~pl[pl < 0], 1)
        assert got == want, c                                            # place[] of a chunk: a bijection onto its addresses
    assert (seen_sp == 1).all() and (seen_p[:plan.nnz] == 1).all()
    return s7


@pytest.mark.parametrize('which', ['one', 'ug-1', 'ug+1', '3ug+7'])
def test_scores7_streams_against_brute_force(which):
    lib, E = _lib_and_engine()
    UG = lib.tmf_wmrb_scores7_users_per_group()
    m = {'one': 1, 'ug-1': UG - 1, 'ug+1': UG + 1, '3ug+7': 3 * UG + 7}[which]
    _check(E, lib, m, 300, 20, 6 * m, seed=m, slice_rows=100, empty_user=min(3, m - 1))


def test_scores7_streams_of_a_tiny_catalog_with_small_sub_chunks(monkeypatch):
    """40 items, S = 30: every item is shared by far more than K users of a group (runs of many steps), and 64 slots per
    sub-chunk (also through TMF_S7_SLOTS) cut runs across sub-chunks."""
    lib, E = _lib_and_engine()
    s7 = _check(E, lib, 70, 40, 30, 400, seed=9, slice_rows=13, slots=64)
    assert s7.n_sub > s7.n_slices * s7.n_groups                          # several sub-chunks per chunk
    monkeypatch.setenv('TMF_S7_SLOTS', '64')
    idx, val, R = _problem(70, 40, 30, 400, 9)
    plan = E.InteractionPlan(idx, val, 70, 40)
    wplan = E.WmrbPlan(plan, R, item_slices=2, n_components=128, sliced=True)
    t7 = E.Scores7Plan(plan, wplan, 128, torch.float32, slice_bytes=13 * 512)
    assert t7.slots == 64 and torch.equal(t7.steps, s7.steps) and torch.equal(t7.place, s7.place)
    monkeypatch.setenv('TMF_S7_SLOTS', str(10 ** 6))                     # never above what the library's buffer holds
    assert E.Scores7Plan(plan, wplan, 128, torch.float32).slots == lib.tmf_wmrb_scores7_slots()
