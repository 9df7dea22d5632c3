"""ConvStack's launch sequence against a recorded fixture (CPU only: tests/convstack_trace.py runs the engine on meta
tensors behind a recording proxy of the library).

tests/golden/convstack_trace/trace.json pins, for every route the engine can take (geometry, batch-size switches, precision,
the FDET_* switches, inference, the fused head, replaced saved tensors, a changing batch size), every launch of a pass with its
integer / float arguments and its pointer arguments as first-appearance ordinals, the timer spans bench.py maps to kernels and
the after_block calls the data-parallel buckets hang on: per step the sequence of events by name and a digest over the events
with all their arguments (one case is there in full).  A change to convstack.py that alters any of it shows here before it
reaches a GPU; `python tests/convstack_trace.py --show CASE` prints a full trace to diff against an earlier commit's."""
import json

import pytest

import convstack_trace as T

CASES = T.cases()


@pytest.fixture(scope="module")
def recorded():
    with open(T.FIXTURE) as f:
        return json.load(f)


def _labels(recorded, step):
    return [recorded["names"][i] for i in recorded["outlines"][step[0]]]


def test_the_fixture_holds_exactly_the_cases(recorded):
    assert sorted(recorded["cases"]) == sorted(CASES)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_launch_trace_equals_the_recorded_one(cid, recorded, monkeypatch):
    got = json.loads(json.dumps(T.run_case(CASES[cid], monkeypatch)))
    want = recorded["cases"][cid]
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        have, labels = [T._label(e) for e in g], _labels(recorded, w)
        first = next((i for i, (a, b) in enumerate(zip(have, labels)) if a != b), min(len(have), len(labels)))
        assert have == labels, f"{cid}, step {s}: first difference at event {first}: got {have[first:first + 2]}, recorded {labels[first:first + 2]}"
        assert len(g) == w[1]
        assert T.digest(g) == w[2], f"{cid}, step {s}: the recorded events in the recorded order, but an argument or a pointer's ordinal differs"
    if cid == T.SAMPLE:
        assert got == recorded["sample"]


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_backward_follows_the_precision_of_its_forward(prec, recorded):
    """set_precision() flipped between forward(save=True) and backward(): the pass is the unflipped one."""
    assert recorded["cases"][f"pool64_480_N2_{prec}_flipped"] == recorded["cases"][f"pool64_480_N2_{prec}"]


def test_the_ps_pool_is_dropped_when_the_batch_size_changes(recorded):
    """Two steps at N = 4, then one at N = 3: the second step allocates no PS buffer, the third a full set again."""
    allocs = [_labels(recorded, step)[-1].split() for step in recorded["cases"]["pool64_480_steps_4_4_3"]]
    assert [a[0] for a in allocs] == ["@ps_alloc"] * 3
    assert int(allocs[0][1]) > 0 and int(allocs[1][1]) == 0 and allocs[2][1] == allocs[0][1]
