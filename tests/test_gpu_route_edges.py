"""k_route at the edges of its bookkeeping (one wave per patch, 256 events per step in four sub-steps of 64, ranks from
ballots): the hand-built calls of tests/plumbing_cases.py, each held to the oracle's loop AND to the plain numpy
selection -- equal index lists, equal `next`.  Dense chunks keep the ballots full, so `taken` grows past the quota
inside a step, the lane that sets `next` is the last of a sub-step, the last of a step or the first of the next one,
and the last lane's mask is all 63 lower bits; the sparse chunks put one event per sub-step at lane 0 or lane 63.
tests/test_plumbing_cases_cpu.py shows on the CPU that every call reaches what it is named after."""
import numpy as np
import pytest

import plumbing_cases as K

pytestmark = pytest.mark.gpu

CHUNKS, CALLS = K.route_calls()


@pytest.fixture(scope="module")
def ctx(ebo):
    with ebo.Context(image_w=240, image_h=180) as c:
        yield c


@pytest.fixture(scope="module")
def loaded(ctx):
    """Loads a chunk unless it is the one the context already holds."""
    state = {"key": None}

    def load(key):
        if state["key"] != key:
            ctx.route_set_events(CHUNKS[key])
            state["key"] = key
        return CHUNKS[key]
    return load


def assert_routed(got, nxt, want, wnxt, what):
    assert len(got) == len(want), what
    for p in range(len(want)):
        assert np.array_equal(got[p], want[p]), (what, p)
    assert np.array_equal(nxt, wnxt), what


@pytest.mark.parametrize("call", CALLS, ids=[c["name"] for c in CALLS])
def test_route_call_matches_oracle_and_plain_selection(ctx, loaded, orc, call):
    ev = loaded(call["chunk"])
    args = (call["rects"], call["start"], call["take"], call["cap"])
    got, nxt = ctx.route_events(*args)
    assert_routed(got, nxt, *orc.route_events(ev, *args), what="oracle")
    assert_routed(got, nxt, *K.route_select(ev, *args), what="selection")


def test_route_second_call_from_the_first_calls_next(ctx, loaded, orc):
    first, moved = K.second_call()
    ev = loaded(first["chunk"])
    got, nxt = ctx.route_events(first["rects"], first["start"], first["take"], first["cap"])
    assert_routed(got, nxt, *orc.route_events(ev, first["rects"], first["start"], first["take"], first["cap"]), what="first")
    got2, nxt2 = ctx.route_events(moved, nxt, first["take"], first["cap"])
    assert_routed(got2, nxt2, *orc.route_events(ev, moved, nxt, first["take"], first["cap"]), what="oracle")
    assert_routed(got2, nxt2, *K.route_select(ev, moved, nxt, first["take"], first["cap"]), what="selection")
