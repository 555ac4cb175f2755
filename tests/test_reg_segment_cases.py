"""The cases of test_gpu_reg_segments.py reach the edges they exist for, and wrong kernels would fail on them (CPU: NumPy alone, no
library loaded).

_reg_segment_cases.walk restates the kernels' walk over the segment table -- thread t takes the vectors t, t + grid * 256, ..., keeps
the segment of its previous vector in a cursor and skips the search while `e0 + 3 < cur.end` -- and is held here to the true segment
of every element.  The same walk is then seeded with five faults; each must change (coef, mask) of some element, the bits of the
restated SGD result, the exact reg_sumsq sums, and Adam's parameter by at least 100 times the bound the GPU test allows."""
import numpy as np
import pytest

import _reg_segment_cases as RS


@pytest.fixture(scope="module")
def big():
    case = RS.build("big")
    got, counts = RS.walk(case)
    return case, got, counts


def test_the_kernel_constants_are_read_from_the_source(repo_root):
    c = RS.kernel_constants(repo_root)
    assert (c["NUM_CU"], c["BLOCKS_PER_CU"], c["MAX_SEGS"]) == (256, 8, 1024)        # the cases were sized for these values
    assert RS.S == c["NUM_CU"] * c["BLOCKS_PER_CU"] * 256 * 4
    for name in ("big", "one", "small"):
        case = RS.build(name)
        assert case.grid == RS.grid_blocks(case.n, c["NUM_CU"], c["BLOCKS_PER_CU"])
    # the grid cap decides when a thread takes a second vector: up to S elements every case so far made one pass
    assert RS.grid_blocks(10007) == 11 and RS.grid_blocks(RS.S) == 2048 and RS.grid_blocks(2098179) == 2048
    assert RS.l2_reg_blocks(RS.build("big").n) == 1024 and -(-RS.build("big").n // (1024 * 256)) == 25


def test_the_layout_is_the_one_described(big):
    case, _, _ = big
    n, st, nm = case.n, case.start, case.named
    assert n == 3 * RS.S + 3111 and case.nseg == 1024 and case.grid == 2048
    assert (n >> 2) == 3 * (RS.S >> 2) + 777 and n - ((n >> 2) << 2) == 3                       # a fourth pass of 777 threads, a tail of 3
    assert list(st[:4]) == [0, 6, 18, 20] and list(np.diff(st[3:11])) == [1, 1, 1, 1, 2, 3, 3]
    a0, a1 = st[nm["A"]], st[nm["A"] + 1]
    c0, c1 = st[nm["C"]], st[nm["C"] + 1]
    assert a0 == 32 and a1 - a0 > RS.S and a1 % 4 == 3 and st[nm["B"] + 1] % 4 == 0 and c0 == st[nm["B"] + 1]
    assert c1 - c0 > RS.S and c1 % 4 == 1
    short = np.diff(st[nm["short0"]:nm["D"] + 1])
    assert len(short) >= 1000 and short.min() == 1 and short.max() == 9
    assert st[nm["last"]] == n - 2 and st[nm["D"] + 1] == n - 2 and st[nm["D"]] < (n >> 2) << 2 < n - 2
    frozen = case.seg_mask == 0
    assert 4 <= frozen.sum() <= 10 and frozen[nm["C"]] and not case.seg_coef[frozen].any()
    assert set(np.unique(case.seg_coef)) == {0.0, 0.25, 0.5, 0.75, 1.0}
    assert ((case.seg_coef == 0) & ~frozen).any()                                                # trainable without a regulariser too
    for name in ("one", "small", "over"):
        other = RS.build(name)
        assert other.nseg == {"one": 1, "small": 9, "over": 1025}[name]
    assert RS.build("one").n == 4 * RS.S + 1 and RS.build("small").n == RS.build("over").n == 10007


def test_the_walk_assigns_every_element_its_segment_and_reaches_the_edges(big):
    case, got, k = big
    np.testing.assert_array_equal(got, case.true_seg)
    for name in ("one", "small"):
        other = RS.build(name)
        np.testing.assert_array_equal(RS.walk(other)[0], other.true_seg)
    print("walk over %d vectors in %d passes: first search %d, fast path %d, re-search after a stale cursor %d, three or more segments "
          "in a vector %d, tail %d" % (k["vectors"], k["passes"], k["first"], k["fast"], k["stale"], k["three_or_more"], k["tail"]))
    assert k["passes"] == 4 and k["first"] == 2048 * 256 and k["first"] + k["fast"] + k["stale"] == k["vectors"]
    assert k["fast"] >= 100000
    assert k["stale"] >= 1000 and k["three_or_more"] >= 50 and k["tail"] == 3
    nm, st = case.named, case.start
    # either side of A's end (3 mod 4: lanes 0-2 in A, lane 3 in B) and of C's end (1 mod 4: lane 0 in C)
    for seg, lanes_inside in (("A", 3), ("C", 1)):
        end = int(st[nm[seg] + 1])
        i = end >> 2
        assert end - 4 * i == lanes_inside
        assert k["fast_vec"][i - 1] and not k["fast_vec"][i] and k["stale_from"][i] == nm[seg], seg
        assert list(got[4 * i:4 * i + 4] == nm[seg]) == [True] * lanes_inside + [False] * (4 - lanes_inside)
        assert not k["fast_vec"][i + 1] and k["stale_from"][i + 1] == nm[seg]
    # the threads arrive in the short segments, and in D's last pass, with a cursor left in C
    s0 = int(st[nm["short0"]])
    assert (k["stale_from"][(s0 >> 2) + 1:int(st[nm["D"]]) >> 2] == nm["C"]).all()
    assert (k["stale_from"][3 * (RS.S >> 2):] == nm["C"]).all()
    tail = got[(case.n >> 2) << 2:]
    assert list(tail) == [nm["D"], nm["last"], nm["last"]]                                     # a tail element in each of the last two
    # one segment: every vector after a thread's first takes the fast path
    one = RS.build("one")
    k1 = RS.walk(one)[1]
    assert (k1["passes"], k1["fast"], k1["stale"], k1["tail"]) == (4, 3 * (RS.S >> 2), 0, 1)
    ks = RS.walk(RS.build("small"))[1]
    assert (ks["passes"], ks["fast"], ks["stale"]) == (1, 0, 0)                                 # what the 10 007-element tests reach


@pytest.fixture(scope="module")
def truth(big):
    """The restated results of the true table on the dense data (config "plain") and the exact sums on the sparse data."""
    case = big[0]
    d = RS.dense_data("big")
    coef, mask = case.coef, case.mask
    sgd = RS.sgd_exact(d["p"], d["g"], None, coef, mask)[0]
    adam = RS.adam_exact(d["p"], d["g"], d["m"], d["v"], None, coef, mask)
    ams = RS.adam_exact(d["p"], d["g"], d["m"], d["v"], d["vhat"], coef, mask)
    w, g = RS.sparse_data("big")
    return dict(sgd=sgd, adam=adam, ams=ams, sums=RS.reg_sums(w, g, coef, mask)[:2])


@pytest.mark.parametrize("mutant", RS.MUTANTS)
def test_a_seeded_fault_in_the_walk_would_fail(big, truth, mutant):
    case = big[0]
    got, _ = RS.walk(case, mutant)
    coef, mask = case.seg_coef[got], case.seg_mask[got]
    wrong = np.flatnonzero((coef != case.coef) | (mask != case.mask))
    assert len(wrong) >= 1
    d = {key: a[wrong] for key, a in RS.dense_data("big").items()}      # (the updates are elementwise: the other elements cannot differ)
    coef_w, mask_w = coef[wrong], mask[wrong]
    sgd = RS.sgd_exact(d["p"], d["g"], None, coef_w, mask_w)[0]
    assert (sgd.astype(np.float32).view(np.int32) != truth["sgd"][wrong].astype(np.float32).view(np.int32)).any()
    w, g = RS.sparse_data("big")
    assert RS.reg_sums(w, g, coef, mask)[:2] != truth["sums"]
    ratios = {}
    for key, vhat in (("adam", None), ("ams", d["vhat"])):
        p_true, _, _, _, upd = truth[key]
        p_mut = RS.adam_exact(d["p"], d["g"], d["m"], d["v"], vhat, coef_w, mask_w)[0]
        ratios[key] = np.abs(p_mut - p_true[wrong]) / RS.adam_bound(d["p"], upd[wrong])
    near = RS.build("big").near()[wrong]
    print("%s: %d wrong elements (%d near a boundary); error / bound over the ones near a boundary: Adam min %.0f, AMSGrad min %.0f; "
          "over all: Adam min %.0f median %.0f, AMSGrad min %.0f median %.0f"
          % (mutant, len(wrong), near.sum(), ratios["adam"][near].min(), ratios["ams"][near].min(), ratios["adam"].min(),
             np.median(ratios["adam"]), ratios["ams"].min(), np.median(ratios["ams"])))
    # a fault that moves a single element, or a few, moves one near a boundary: there the data make every wrong (coef, mask) visible
    assert near.any()
    for r in ratios.values():
        assert r[near].min() >= 100.0
        if len(wrong) <= 16:
            assert near.all() and r.min() >= 100.0


def test_the_sparse_sums_are_exact_in_float32():
    for name in ("big", "one", "small"):
        case = RS.build(name)
        w, g = RS.sparse_data(name)
        assert set(np.unique(w)) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and set(np.unique(g)) <= {-1.0, 0.0, 1.0}
        on = case.near()
        assert (w[on] != 0).all() and (g[on] != 0).all() and (w[~on] != 0).sum() >= (case.n // 97) - on.sum()
        for mask in (case.mask, np.ones(case.n, np.float32)):
            loss, norm, units = RS.reg_sums(w, g, case.coef, mask)
            print(name, "loss %g gnorm_sq %g: %d units of 1/4" % (loss, norm, units))
            assert loss > 0 and norm > 0 and units < 2 ** 24 and loss * 4 == int(loss * 4) and norm * 4 == int(norm * 4)


def test_the_dense_data_are_exact_and_the_restatement_notices_data_that_are_not():
    for name in ("big", "small"):
        case, d = RS.build(name), RS.dense_data(name)
        frozen = case.mask == 0
        assert frozen.any() and (d["p"] != 0).all() and (np.abs(d["p"]) <= 4).all() and (d["p"] * 8 == np.round(d["p"] * 8)).all()
        for key in ("vel", "m", "v", "vhat"):
            assert (d[key][~frozen] != 0).all() and not d[key][frozen].any()
        assert (d["v"] >= 0).all() and (d["vhat"] > d["v"]).any() and (d["vhat"] < d["v"]).any()
    case, d = RS.build("small"), RS.dense_data("small")
    for cfg in RS.CONFIGS.values():                                      # two steps of every SGD kind and one of Adam stay exact
        for nesterov in (False, True):
            p, vel = RS.sgd_exact(d["p"], d["g"], d["vel"], case.coef, case.mask, nesterov, **cfg)
            RS.sgd_exact(p, d["g2"], vel, case.coef, case.mask, nesterov, **cfg)
        RS.adam_exact(d["p"], d["g"], d["m"], d["v"], d["vhat"], case.coef, case.mask, **cfg)
    with pytest.raises(AssertionError, match="no float32 number"):
        RS.sgd_exact(d["p"] + np.float32(2.0 ** -22), d["g"], d["vel"], np.full(case.n, 1.0 / 3), case.mask)
