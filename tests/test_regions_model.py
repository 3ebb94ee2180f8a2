"""The argument behind oge_filter_regions_dev, checked on the Python model alone: the regions sorted by
(ref_id, left_pos) with the running maximum of right_pos answer "does at least one region hold" with one binary
search per record, for any list -- overlapping, nested, duplicate, touching, inverted (left > right) regions,
ref_id -1, and positions whose pos + l_seq wraps."""
import random

import pytest

import regions_model as R

I32 = (1 << 31) - 1


def random_regions(rng, n, n_ref):
    out = []
    for _ in range(n):
        ref = rng.choice([-1, *range(n_ref), n_ref + 3])
        a, b = rng.randrange(-50, 3000), rng.randrange(-50, 3000)
        kind = rng.randrange(6)
        if kind == 0 and out:
            out.append(rng.choice(out))                      # duplicate
        elif kind == 1 and out:
            r = rng.choice(out)
            out.append((r[0], r[2] + 1, r[2] + rng.randrange(1, 40)))  # touching its right end
        elif kind == 2:
            out.append((ref, max(a, b), min(a, b)))          # inverted when a != b
        elif kind == 3:
            out.append((ref, a, a))                          # one position
        else:
            out.append((ref, min(a, b), max(a, b)))
    return out


@pytest.mark.parametrize("n_regions", [1, 2, 7, 64, 300])
def test_search_equals_the_loop_over_the_regions(n_regions):
    rng = random.Random(n_regions)
    regions = random_regions(rng, n_regions, 4)
    keys, rmax = R.sorted_running_max(regions)
    assert keys == sorted(keys)
    for _ in range(4000):
        refid = rng.choice([-1, 0, 1, 2, 3])
        pos = rng.choice([rng.randrange(-2, 3100), I32 - rng.randrange(0, 40), -1])
        lseq = rng.choice([0, 1, rng.randrange(0, 200), 100])
        want = any(R.in_region(refid, pos, lseq, r) for r in regions)
        assert R.in_regions_by_search(refid, pos, lseq, keys, rmax) == want, (refid, pos, lseq)


def test_wrapping_end_is_the_filters():
    # pos + l_seq past 2^31 - 1 wraps to a negative end, as the single-region Filter's int arithmetic does
    assert not R.in_region(0, I32 - 5, 100, (0, 0, I32))
    assert R.in_region(0, I32 - 5, 100, (0, -(1 << 31), I32))
