"""The index arithmetic of the device rings that the output iterations of lbm_step fill and the drains empty (body-force log, frames,
probes: csrc/lbm_plan.hpp RingIndex), through lbm_debug_ring: no device. A push answers with its slot, or "full"; a take of up to m
answers with the two pieces it copies, slots [start, start + n1) and then [0, n2). Held against a model made of two deques — the free
slots in the order they come round, and the pending ones — which never computes an index."""
import collections
import importlib
import random

import pytest

from tests.helpers import PKG

PUSH = -1
CAPACITIES = (1, 2, 3, 7)


@pytest.fixture(scope="module")
def ring():
    pkg = importlib.import_module(PKG)
    pkg.build_all()
    return pkg.debug_ring


def check(ring, cap, ops):
    got, left = ring(cap, ops)
    free, pending = collections.deque(range(cap)), collections.deque()
    for k, (op, (a, b, c)) in enumerate(zip(ops, got.tolist())):
        where = (cap, k, op)
        if op == PUSH:
            assert (b, c) == (-1, -1), where
            if free:
                pending.append(free.popleft())
                assert a == pending[-1], where
            else:
                assert a == -1 and len(pending) == cap, where      # full: refused, nothing changes
        else:
            taken = [pending.popleft() for _ in range(min(op, len(pending)))]
            free.extend(taken)
            assert b >= 0 and c >= 0 and 0 <= a and a + b <= cap, where
            assert list(range(a, a + b)) + list(range(c)) == taken, where      # oldest first, two contiguous pieces
            assert c == 0 or a + b == cap, where                               # the second piece only behind the buffer's end
    assert left == len(pending)
    return got.tolist()


def edge_ops(n):
    """fill, push on full, take 0, a partial take, take more than pending (which ends exactly at the end of the buffer), then a full
    ring whose head is the last slot (a take of 1 + (n - 1)) and one whose head is slot 1 ((n - 1) + 1)."""
    ops = [PUSH] * n + [PUSH, 0, n // 2, 100 * n]
    ops += [PUSH] * n + [n - 1] + [PUSH] * (n - 1) + [n]
    ops += [PUSH, 1, PUSH, 1] + [PUSH] * n + [PUSH, n, 0, 5]
    return ops


@pytest.mark.parametrize("cap", CAPACITIES)
def test_the_edge_cases_agree_with_the_deque(ring, cap):
    check(ring, cap, edge_ops(cap))


def test_the_edge_cases_of_seven_slots_spelled_out(ring):
    got = check(ring, 7, edge_ops(7))
    takes = [tuple(g) for op, g in zip(edge_ops(7), got) if op != PUSH]
    assert takes == [(0, 0, 0), (0, 3, 0), (3, 4, 0),      # take 0; a partial take; more than pending, up to the buffer's end
                     (0, 6, 0), (6, 1, 6),                 # 1 + (n - 1)
                     (6, 1, 0), (0, 1, 0), (1, 6, 1),      # (n - 1) + 1
                     (1, 0, 0), (1, 0, 0)]                 # an empty ring gives nothing
    pushes = [g[0] for op, g in zip(edge_ops(7), got) if op == PUSH]
    assert pushes == [0, 1, 2, 3, 4, 5, 6, -1] + [0, 1, 2, 3, 4, 5, 6] + [0, 1, 2, 3, 4, 5] + [6, 0] + [1, 2, 3, 4, 5, 6, 0, -1]


@pytest.mark.parametrize("cap", CAPACITIES)
def test_random_sequences_agree_with_the_deque(ring, cap):
    rng = random.Random(20240 + cap)
    for _ in range(4):
        ops = [PUSH if rng.random() < 0.6 else rng.randint(0, cap + 2) for _ in range(300)]
        check(ring, cap, ops)


def test_bad_arguments_are_refused(ring):
    pkg = importlib.import_module(PKG)
    with pytest.raises(pkg.LbmError):
        ring(0, [PUSH])
    assert ring(3, [])[1] == 0
