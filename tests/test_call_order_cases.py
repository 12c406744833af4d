"""The builders of call_order_cases.py, without a device: what makes the GPU
tests of test_gpu_call_order.py mean something. For every entry point the
primers are larger than every target in each dimension the checker sizes a
buffer by, the dirty primer is invalid by its reference with lists longer than
any cap a target is called with, the clean primer is valid, and every target's
reference answer is the one the case is named for."""
import pytest

import call_order_cases as K
from jepsen_amd import _abi as A


@pytest.fixture(scope="module", params=K.NAMES)
def entry(request):
    return K.BY_NAME[request.param]


def first_path(e, case):
    return e.paths_of(case)[0]


def test_every_entry_point_of_the_header_is_here():
    flat = {"counter", "set", "set-bitmaps", "set-full", "total-queue", "queue", "unique-ids", "bank", "long-fork",
            "causal-reverse", "scc", "cycle", "cycle-append", "cycle-mono", "causal", "g2", "perf"}
    assert set(K.NAMES) == flat == set(K.STAGES)
    assert [e.name for e in K.ENTRIES] == K.NAMES


def test_primers_exceed_every_target_in_each_dimension(entry):
    c = entry.cases()
    for primer in (c["dirty"], c["clean"]):
        big = entry.dims(primer)
        for t in c["targets"]:
            small = entry.dims(t)
            assert set(small) == set(big)
            for k, v in small.items():
                if k in entry.capped or k == "runs" or (k in entry.error_dims and primer.name == "clean"):
                    continue                                    # the output lists: the next test; a clean primer has no errors
                assert big[k] > v, (entry.name, primer.name, t.name, k, big[k], v)


def test_dirty_primer_is_invalid_with_lists_above_every_target_cap(entry):
    c = entry.cases()
    dirty, clean = c["dirty"], c["clean"]
    full = entry.full(dirty, first_path(entry, dirty))
    assert not entry.valid(full)
    assert full.get("valid", A.INVALID) == A.INVALID and full.get("valid?", False) is False      # not :unknown either
    lens = entry.lists(full)
    clean_lens = entry.lists(entry.full(clean, first_path(entry, clean)))
    for t in c["targets"]:
        for k, cap in entry.caps(t, first_path(entry, t)).items():
            have = clean_lens[k] if k in entry.clean_only else lens[k]
            assert have > cap, (entry.name, t.name, k, have, cap)
    # two tiles of the checker and an odd remainder, and no more than about 13k rows
    assert 4096 < entry.dims(dirty)["rows"] <= 13_000 and 4096 < entry.dims(clean)["rows"] <= 13_000


def test_clean_primer_is_valid_with_empty_error_lists(entry):
    clean = entry.cases()["clean"]
    full = entry.full(clean, first_path(entry, clean))
    assert entry.valid(full)
    for k, n in entry.lists(full).items():
        if k in ("reads", "pair", "pt_row", "series", "cells", "edges", "runs", "never-read") or k in entry.clean_only:
            continue                                            # results, not errors
        assert n == 0, (entry.name, k, n)


def test_targets_have_the_edges_and_the_answers_they_are_named_for(entry):
    c = entry.cases()
    names = [t.name for t in c["targets"]]
    assert len(names) == len(set(names)) and "n0" in names and "n1" in names
    assert {"dirty", "clean"}.isdisjoint(names)
    rows = {t.name: entry.dims(t)["rows"] for t in c["targets"]}
    assert rows["n0"] == 0 and rows["n1"] == 1
    edges = sorted(n for n in names if n.startswith(("T-1", "T+0", "T+1", "T", "ring-N")))
    assert len(edges) >= 3, (entry.name, names)
    for t in c["targets"]:
        for path in entry.paths_of(t):
            full = entry.full(t, path)
            assert entry.want(t, path) == full                 # a target's caps cut nothing of its own
    empty = entry.full(entry.target("n0"), first_path(entry, entry.target("n0")))
    for k, n in entry.lists(empty).items():
        assert n == 0, (entry.name, k)


HAND = {
    "g2": {"single-key-illegal": ("illegal", [[0, 2]]), "unsorted-ids": ("illegal", [[0, 2], [1, 2], [2, 2]]),
           "T+0": ("illegal", [[0, 2], [A.G2_TILE - 1, 2]]), "T+1-legal": ("legal_count", A.G2_TILE + 1)},
    "unique-ids": {"all-nil": ("duplicated", [[None, 3]]), "one-duplicate": ("duplicated", [[-12345678901, 2]]),
                   "fail-info-carry-an-acked-id": ("range", [4, 9])},
    "scc": {"two-sccs-trivial-between": ("sccs", [[1, 2], [3, 4]]), "two-cycles-63-64-255-256": ("sccs", [[63, 64], [255, 256]]),
            "ring-N": ("sccs", [list(range(A.CY_LDS_VERTICES))])},
    "queue": {"S-3-clean": ("valid", A.VALID)},
    "set": {"never-read": ("valid", A.UNKNOWN), "T": ("valid", A.VALID), "T+1-lost": ("lost_count", 2)},
    "counter": {"T+0": ("n_errors", 0), "n1": ("n_reads", 0)},
    "cycle": {"two-writers-read": ("cause", A.CAUSE_MULTIPLE_WRITES), "double-invoke": ("unknown_row", 1),
              "healthy": ("valid", A.VALID), "cycles": ("valid", A.INVALID)},
    "perf": {"unpaired": ("n_unpaired_invokes", 1)},
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_pinned_target_answers(name):
    e = K.BY_NAME[name]
    for case, (field, value) in HAND[name].items():
        t = e.target(case)
        assert e.full(t, first_path(e, t))[field] == value, (name, case, field)


def test_hand_written_cases_of_the_modules_are_targets():
    import bank_cases, causal_cases, causal_reverse_cases, g2_cases, long_fork_cases, perf_cases
    for name, cases, skip in (("bank", bank_cases.CASES, ()), ("g2", g2_cases.CASES, ("empty", "no-inserts")),
                              ("long-fork", long_fork_cases.CASES, long_fork_cases.HOST_ONLY),
                              ("perf", perf_cases.CASES, ())):
        have = {t.name for t in K.BY_NAME[name].cases()["targets"]}
        missing = {c for c in cases if c not in skip and cases[c]} - have
        assert not missing or name == "perf" and all(not perf_cases.CASES[m] for m in missing), (name, missing)
    assert len(K.BY_NAME["causal"].cases()["targets"]) > 20 and len(K.BY_NAME["causal-reverse"].cases()["targets"]) > 15


def test_the_chain_covers_every_entry_point_and_alternates_sizes():
    fwd, rev = K.chain(False), K.chain(True)
    assert [e.name for e, _ in fwd] == K.NAMES and [e.name for e, _ in rev] == K.NAMES[::-1]
    for order in (fwd, rev):
        big = [c.name in ("dirty", "clean") for _, c in order]
        assert big[0] and all(a != b for a, b in zip(big, big[1:]))


def test_handoffs_follow_larger_staged_columns():
    """Every checker that stages no key (no aux) has large keyed (aux-carrying)
    calls to follow, each with more rows (aux) than the targets run after it."""
    assert set(K.HANDOFFS) == {n for n, st in K.STAGES.items() if st is not None and not all(st)}
    for name, stagers in K.HANDOFFS.items():
        e = K.BY_NAME[name]
        need_key, need_aux = K.STAGES[name]
        assert (need_key or set(K.KEYED) <= set(stagers)) and (need_aux or set(K.AUXED) <= set(stagers))
        for s in stagers:
            big = K.BY_NAME[s].cases()["dirty"].cols
            assert K.STAGES[s][0] and big.n_keys > 0 or s in K.AUXED
            for t in e.cases()["targets"]:
                if t.name in ("n1", "T+1"):
                    assert big.n > t.cols.n, (name, s, t.name)
                    if s in K.AUXED and not need_aux:
                        assert len(big.aux) > t.cols.n
