"""The inputs of test_gpu_detect_edges.py hold what they claim (CPU: the host references alone, no library loaded).

Each case of _detect_cases.py exists for one edge of csrc/detect.hip's index arithmetic; the claims that put it on that edge -- a box in
the third 256-wide x block, ones in the rows of the second grid-stride pass, 129 taps, an invalid id on a wave's last lane, a maximum in
the lane loop's last pass only -- are asserted here, together with the agreement of the two host restatements of unmold_mask on every
paste case, so a re-seeded or edited case that has left its edge is red wherever the suite runs."""
import numpy as np
import pytest

import _detect_cases as K
import _maskrcnn_ref as R

F32 = np.float32


# ---- class_select ------------------------------------------------------------------------------------------------------------------

def test_select_sweep_covers_the_lane_loop_and_block_edges():
    passes = {C: -(-C // K.CS_LANES) for C in K.SELECT_C}
    assert passes == {63: 1, 64: 1, 65: 2, 128: 2, 129: 3, 200: 4}
    assert [C % K.CS_LANES for C in (65, 129)] == [1, 1]                             # a lone element in the last pass
    assert [R_ % K.CS_ROWS for R_ in K.SELECT_R] == [0, 1, 3] and min(K.SELECT_R) == K.CS_ROWS
    for C in K.SELECT_C:
        for R_ in K.SELECT_R:
            z, d = K.select_case(R_, C)
            assert z.shape == (R_, C) and d.shape == (R_, 4 * C) and np.isfinite(z).all()
            assert np.array_equal(R.class_select(z, d)[0][:2], [0, C - 2])           # the planted neighbour ties resolve downwards
            assert K.select_finite_gap(z) == R.class_select(z, d)[3]


@pytest.mark.parametrize("C", K.SELECT_C)
def test_select_planted_rows_resolve_as_stated(C):
    z, d, names, want = K.select_planted(C)
    expect = ["last_only"] + {200: ["tie_5_69_133"], 65: ["tie_64_1"]}.get(C, []) + (["tie_63_64"] if C >= 65 else []) \
        + (["only_70_finite"] if C > 70 else []) + ["neg_inf_at_0"]
    assert names == expect
    assert not np.isnan(z).any() and not np.isposinf(z).any() and np.isfinite(z).any(axis=1).all()
    ids, scores, dd, d_max = R.class_select(z, d)
    assert np.array_equal(ids, want) and np.isfinite(scores).all()
    for n, name in enumerate(names):
        row, top = z[n], z[n].max()
        hits = np.flatnonzero(row == top).tolist()
        if name == "last_only":
            assert hits == [C - 1] and want[n] == C - 1
        elif name == "tie_5_69_133":
            assert hits == [5, 69, 133] and len({h % K.CS_LANES for h in hits}) == 1 and want[n] == 5
        elif name == "tie_64_1":
            assert hits == [1, 64] and want[n] == 1                                 # the lower lane holds the HIGHER index
        elif name == "tie_63_64":
            assert hits == [63, 64] and want[n] == 63
        elif name == "only_70_finite":
            assert np.flatnonzero(np.isfinite(row)).tolist() == [70] and want[n] == 70 and scores[n] == 1.0
        else:
            assert np.isneginf(row[0]) and np.isfinite(row[1:]).all() and want[n] >= 1 and hits == [want[n]]
        assert np.array_equal(dd[n], d[n, 4 * want[n]:4 * want[n] + 4])
    assert np.isfinite(K.select_finite_gap(z)) and (np.isinf(d_max) or d_max == K.select_finite_gap(z))


# ---- mask_head_tail ------------------------------------------------------------------------------------------------------------------

def test_tail_edges_are_the_stated_shapes():
    shapes = {n: v[:5] for n, v in K.TAIL_EDGES.items()}
    assert shapes == {"single_pixel": (1, 1, 32, 32, 2), "lane_per_roi": (1, 70, 96, 96, 70), "max_p_four_blocks": (16, 2, 160, 64, 5),
                      "cin_below_cmid": (7, 3, 32, 256, 81), "cin_above_cmid": (7, 3, 256, 32, 81), "rows_128": (4, 8, 224, 96, 5),
                      "rows_144": (4, 9, 224, 96, 5), "all_invalid": (14, 3, 128, 128, 5), "invalid_first": (14, 3, 64, 32, 5),
                      "invalid_last": (14, 3, 64, 32, 5), "off_boundary": (7, 3, 96, 96, 5)}
    rows = {n: v[1] * v[0] * v[0] for n, v in K.TAIL_EDGES.items()}
    assert rows["single_pixel"] == 1 and rows["max_p_four_blocks"] == 4 * K.MT_ROWS and rows["rows_128"] == K.MT_ROWS
    assert rows["rows_144"] == K.MT_ROWS + 16 and rows["cin_below_cmid"] == rows["cin_above_cmid"] == 147
    signed = [n for n, v in K.TAIL_EDGES.items() if v[5]]
    assert 2 * len(signed) >= len(K.TAIL_EDGES) - 1                                  # half of the cases are not post-ReLU
    for n in K.TAIL_EDGES:
        x = K.tail_edge(n)[0]
        assert (x.min() < -1.0) == (n in signed) and x.max() > 1.0


def test_tail_invalid_ids_sit_where_stated():
    def bad(name):
        ids, C = K.tail_edge(name)[5].astype(np.int64), K.TAIL_EDGES[name][4]
        return np.flatnonzero((ids < 0) | (ids >= C)).tolist(), ids
    rows, ids = bad("lane_per_roi")                                                  # P = 1: RoI n is row n
    assert rows == [0, 31, 32, 69] and ids[[0, 31, 32, 69]].tolist() == [-1, 70, K.INT_MAX, K.INT_MIN]
    assert rows[0] % K.MT_WAVE_ROWS == 0 and rows[1] % K.MT_WAVE_ROWS == K.MT_WAVE_ROWS - 1 and rows[2] == K.MT_WAVE_ROWS and rows[3] == len(ids) - 1
    valid = np.delete(ids, rows)
    assert np.array_equal(valid, np.delete(np.arange(70), rows))                      # every other lane has its own class column
    assert bad("all_invalid")[0] == [0, 1, 2] and bad("invalid_first")[0] == [0] and bad("invalid_last")[0] == [2]
    for n in set(K.TAIL_EDGES) - {"lane_per_roi", "all_invalid", "invalid_first", "invalid_last"}:
        assert bad(n)[0] == [], n
    ids = K.tail_edge("cin_below_cmid")[5]
    assert 0 in ids and 80 in ids                                                    # the first and the last class column


@pytest.mark.parametrize("name", list(K.TAIL_EDGES))
def test_tail_case_exercises_the_relu_and_leaves_the_sigmoid_unsaturated(name):
    y = K.tail_pre_relu(name)
    P, N, Cin, Cmid, C = K.TAIL_EDGES[name][:5]
    assert y.shape == (N * P * P, 4 * Cmid)
    assert (y < 0).mean() >= 0.1 and (y > 0).mean() >= 0.1
    out, z, A = K.tail_reference(name)
    assert np.abs(z).max() < 30.0
    ids = K.tail_edge(name)[5].astype(np.int64)
    ok = (ids >= 0) & (ids < C)
    assert (A[ok] > 0).all() and not A[~ok].any() and not out[~ok].any()
    assert ((out[ok] > 0) & (out[ok] < 1)).all()


# ---- mask_paste ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", K.PASTE_NAMES)
def test_paste_references_agree(name):
    """mask_rcnn_model.unmold_mask (PIL) equals the independent integer restatement on every detection of every case."""
    c = K.paste_case(name)
    want = c.reference()
    assert want.shape == (c.M, c.H, c.W) and want.dtype == np.uint8 and want.max() <= 1
    for i in range(c.M):
        assert np.array_equal(want[i], R.unmold_mask(c.masks[i], c.boxes[i], (c.H, c.W, 3))), (name, c.labels[i])
    m = c.masks
    assert np.isfinite(m).all() and ((m == 0) | (np.abs(m) >= np.finfo(F32).tiny)).all()
    assert ((m.max(axis=(1, 2)) - m.min(axis=(1, 2))).astype(np.float64) >= 1e-30).all()


def test_paste_blocks_case_reaches_every_x_block():
    c = K.paste_case("blocks_300x521")
    assert (c.H, c.W) == (300, 521) and -(-c.W // K.MP_THREADS) == 3 and c.W % K.MP_THREADS != 0 and c.masks.shape[1:] == (28, 28)
    b = {n: c.boxes[i].tolist() for i, n in enumerate(c.labels)}
    want = c.reference()
    assert b["full"] == [0, 0, 300, 521]
    assert b["across_256"][1] < 256 < b["across_256"][3] < 512 and b["past_512"][1] > 512
    for n, x1, w in (("w256_at_0", 0, 256), ("w257_at_0", 0, 257), ("w256_at_255", 255, 256), ("w257_at_255", 255, 257),
                     ("column_256", 256, 1), ("column_520", 520, 1)):
        assert b[n][1] == x1 and b[n][3] - b[n][1] == w, n
    assert b["taller_than_256"][2] - b["taller_than_256"][0] > 256
    assert b["touches_corner"][2:] == [300, 521]
    y1, x1, y2, x2 = b["leaves_in_x"]
    assert x2 == c.W + 1 and 0 <= y1 < y2 <= c.H and 0 <= x1
    for i, n in enumerate(c.labels):
        y1, x1, y2, x2 = c.boxes[i]
        if n == "leaves_in_x":
            assert not want[i].any()
            continue
        inside = want[i, y1:y2, x1:x2]
        assert want[i].sum() == inside.sum() and inside.any() and not inside.all(), n  # ones in the box only, and zeros in it as well
        cols = np.flatnonzero(want[i].any(axis=0))
        if x2 > 256:
            assert cols.max() >= 256, n                                              # ones that only a second x block writes
        if x1 > 512:
            assert cols.min() > 512
    assert want[c.index("full"), :, 512:].any() and want[c.index("full"), 256:, :].any()


def test_paste_tall_and_wide_cases_have_ones_past_the_grid_limit():
    t = K.paste_case("rows_70001x3")
    assert (t.H, t.W, t.M) == (70001, 3, 3) and t.H > K.MP_MAX_GRID
    want = t.reference()
    b = {n: t.boxes[i].tolist() for i, n in enumerate(t.labels)}
    assert b["full"] == [0, 0, 70001, 3] and b["second_pass_only"][0] >= K.MP_MAX_GRID and b["straddles_65535"][0] < K.MP_MAX_GRID < b["straddles_65535"][2]
    for i in range(t.M):
        tail = want[i, K.MP_MAX_GRID:]
        assert tail.any() and not tail.all(), t.labels[i]                            # the second pass writes ones and zeros
        assert want[i, :K.MP_MAX_GRID].any() == (t.labels[i] != "second_pass_only")
    w = K.paste_case("cols_3x70001")
    assert (w.H, w.W, w.M) == (3, 70001, 2) and -(-w.W // K.MP_THREADS) == 274
    want = w.reference()
    for i in range(w.M):
        assert w.boxes[i][3] - w.boxes[i][1] > K.MP_MAX_GRID
        assert want[i, :, K.MP_MAX_GRID:].any() and not want[i, :, K.MP_MAX_GRID:].all() and want[i, :, :K.MP_MAX_GRID].any()


def test_paste_tap_cases_reach_the_longest_windows():
    assert [K.resize_ksize(64, n) for n in (1, 2, 3)] == [129, 65, 45]
    assert K.resize_ksize(28, 28) == 3 and K.resize_ksize(28, 900) == 3 and K.resize_ksize(64, 50) == 5
    sides = {"taps_64x64": (64, 64, K.TAPS_BOXES_64x64), "taps_64x1": (64, 1, K.TAPS_BOXES_64x1), "taps_1x64": (1, 64, K.TAPS_BOXES_1x64)}
    assert K.TAPS_BOXES_64x64 == [(1, 1), (1, 3), (3, 1), (2, 2), (3, 50)]
    for name, (h, w, boxes) in sides.items():
        c = K.paste_case(name)
        assert (c.H, c.W) == (40, 50) and c.masks.shape == (3 * len(boxes), h, w)
        got = [(int(b[2] - b[0]), int(b[3] - b[1])) for b in c.boxes[::3]]
        assert got == boxes
        ks = {K.resize_ksize(h, bh) for bh, _ in boxes} | {K.resize_ksize(w, bw) for _, bw in boxes}
        assert {129, 65, 45} <= ks, (name, ks)                                       # a 64-sample axis onto 1, 2 and 3 outputs
        # the table of one axis: out * (2 + taps) ints, taps at most the source's length -- inside the 2 in + 5 out the kernel reserves
        for n_in, n_out in [(h, bh) for bh, _ in boxes] + [(w, bw) for _, bw in boxes]:
            assert n_out * (2 + min(K.resize_ksize(n_in, n_out), n_in)) <= 2 * n_in + 5 * n_out
        want = c.reference()
        inside = [want[i, b[0]:b[2], b[1]:b[3]] for i, b in enumerate(c.boxes)]
        assert any(v.any() for v in inside) and any(not v.all() for v in inside), name
        assert all(want[i].sum() == inside[i].sum() for i in range(c.M))
        for m in c.masks:
            assert len(np.unique(m)) >= 2                                            # structure: no constant mask


def test_paste_production_case():
    c = K.paste_case("production_1024")
    assert (c.H, c.W, c.M) == (1024, 1024, 1) and c.boxes[0].tolist() == [60, 70, 960, 970]
    want = c.reference()[0]
    assert want[:, 768:].any() and want[768:].any() and 0.05 < want.mean() < 0.6


def test_paste_bytescale_edges_are_what_they_claim():
    from image_captioning_amd import mask_rcnn_model as MR
    c = K.paste_case("bytescale_97x131")
    ulp, negative, ties, again = c.masks
    assert c.labels == ["ulp", "negative", "ties", "ties_identity"] and c.masks.shape == (4, 28, 28) and np.array_equal(ties, again)
    assert sorted(np.unique(ulp).tolist()) == [0.5, 0.5 + 2.0 ** -24] and ulp.max() - ulp.min() == F32(2.0 ** -24)
    assert sorted(np.unique(MR.bytescale(ulp)).tolist()) == [0, 255]
    assert negative.max() < -0.4 and negative.min() < -1.4
    assert ties.min() == 0.0 and ties.max() == F32(255.0 / 2 ** K.TIE_SHIFT)
    scaled = ties.astype(np.float64) * 2.0 ** K.TIE_SHIFT                           # exact: the scale is a power of two
    inner = scaled[(ties != ties.min()) & (ties != ties.max())]
    assert np.array_equal(inner - np.floor(inner), np.full(inner.shape, 0.5)) and len(np.unique(inner)) > 20
    assert int((scaled == 127.5).sum()) >= 36                                        # the tie ON the threshold: byte 128 or 127
    assert np.array_equal(MR.bytescale(ties), np.floor(scaled + 0.5).astype(np.uint8))       # a tie goes up: j + 0.5 -> j + 1
    assert np.array_equal(MR.bytescale(ties), K.tie_bytes(ties, "up"))
    for m in c.masks:
        assert np.array_equal(MR.bytescale(m), R.bytescale(m))
    want = c.reference()
    for i in range(c.M):
        assert want[i].any() and not want[i].all(), c.labels[i]
    # the direction of the rounding reaches the pasted plane: ties taken down give another reference in both boxes (the 127.5 patch
    # falls to 127, below the threshold); ties taken to even leave 127.5 -> 128 alone and show only through the interpolation
    shape = (c.H, c.W, 3)
    for i in (c.index("ties"), c.index("ties_identity")):
        assert np.array_equal(K.paste_bytes(K.tie_bytes(ties, "up"), c.boxes[i], shape), want[i])
        changed = int((K.paste_bytes(K.tie_bytes(ties, "down"), c.boxes[i], shape) != want[i]).sum())
        assert changed >= 36, (c.labels[i], changed)
    i = c.index("ties")
    assert (K.paste_bytes(K.tie_bytes(ties, "even"), c.boxes[i], shape) != want[i]).any()
