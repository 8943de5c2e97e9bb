"""CPU: the scenes of tests/_newpts_scenes.py exercise the chain.  The composed restatement gives the pinned number of new points per
neighbour, at least two neighbours contribute, a neighbour in the middle contributes nothing where the table says so, every feature of
the current keyframe gets at most one point, and the stale-mask batch gives another (larger) total."""
import pytest

import _newpts_scenes as N


@pytest.mark.parametrize("key", sorted(N.ROWS), ids=lambda k: "seed%d-nn%d-n%d-%s" % (k[0], k[1], k[2], "f%d" % k[4] if k[4] else "b%d" % k[3]))
def test_rows_give_the_pinned_counts(key):
    counts, stale = N.ROWS[key]
    ch = N.chain(*key)
    got = ch.per_neighbour()
    assert got == counts
    assert sum(1 for c in got if c > 0) >= 2                                  # the running id crosses a neighbour
    ids = [w[0] for w in ch.want]
    assert ids == list(range(ch.first_id, ch.first_id + sum(counts)))
    feats = [w[2] for w in ch.want]
    assert len(set(feats)) == len(feats)                                      # a feature of the current keyframe: at most one point
    assert not any(ch.has_mp_cur[i] for i in feats)
    assert ch.stale_total() == stale and stale > sum(counts)                  # the stale-mask batch is another answer


def test_a_neighbour_in_the_middle_contributes_nothing():
    counts, _ = N.ROWS[(2, 7, 70, 32, 0)]
    assert counts[3] == 0 and counts[2] > 0 and counts[4] > 0
    assert N.chain(2, 7, 70, 32, 0).per_neighbour()[3] == 0


def test_masks_follow_the_accepted_matches():
    ch = N.chain(1, 3, 40, 32, 0)
    cur, nb = ch.final_masks()
    assert int(cur.sum()) == int(ch.has_mp_cur.sum()) + len(ch.want)
    for k in range(ch.nn):
        assert int(nb[k].sum()) >= int(ch.has_mp_nb[k].sum())
