"""The hand-built banks of tests/nav_edge_banks.py: their tables are consistent, the oracle agrees with the brute-force
definition on every pose the GPU tests use (tests/test_gpu_nav_edges.py compares the kernels with the oracle), and every pose
presents what it is there for -- an exact tie between distant parts of the path, a survivor list too long for registers, a knot
interval the uniform guess misses by intervals.  The conditions are asserted per pose: a case that fails its condition fails."""
import numpy as np
import pytest

import nav_edge_banks as nb

BUILDERS = dict(u32=lambda: nb.u_path(100, 32), u8=lambda: nb.u_path(100, 8), comb=lambda: nb.comb_path(6), stutter=nb.stutter_path,
                knots_two=nb.knots_two, knots_three=nb.knots_three, head=nb.knots_clustered_head, tail=nb.knots_clustered_tail,
                short_last=nb.knots_short_last, **{"line%d" % n: (lambda n=n: nb.straight_path(n)) for n in nb.STRAIGHT_SIZES})


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_tables_are_self_consistent(name):
    bank = BUILDERS[name]()
    xy, cum, knot_s, coef, L = nb.world_tables(bank, 0)
    assert np.all(xy * 8 == np.round(xy * 8))
    seg = np.diff(xy, axis=0)
    assert np.all((seg[:, 0] == 0) | (seg[:, 1] == 0))                        # axis-aligned: lengths are exact
    want = np.concatenate([[0.0], np.cumsum(np.abs(seg).sum(axis=1))])
    np.testing.assert_array_equal(cum, want)
    assert L == cum[-1] == knot_s[-1] and knot_s[0] == 0.0 and np.all(np.diff(knot_s) > 0)
    assert bank["p_max"] == len(xy) and tuple(bank["poly_off"]) == (0, len(xy)) and tuple(bank["knot_off"]) == (0, len(knot_s))
    assert coef.shape == (len(knot_s), 8)
    np.testing.assert_array_equal(bank["world_scalar"][0, :5], [L, xy[-1, 0], xy[-1, 1], xy[0, 0], xy[0, 1]])
    # the spline at every knot, from the left piece and from the right one, is the polyline's point at that arclength
    for i, s in enumerate(knot_s):
        p, _ = nb._piece(xy, cum, s)
        if i < len(knot_s) - 1:
            np.testing.assert_array_equal(nb.spline_eval(knot_s, coef, s)[0], p)
        if i > 0:
            z = s - knot_s[i - 1]
            np.testing.assert_array_equal([coef[i - 1, 3] + coef[i - 1, 2] * z, coef[i - 1, 7] + coef[i - 1, 6] * z], p)
    # ... and at every vertex
    for v in range(0, len(xy), 7):
        np.testing.assert_array_equal(nb.spline_eval(knot_s, coef, cum[v])[0], xy[v])


def test_sizes_named_by_the_cases():
    assert len(nb.world_tables(nb.u_path(100, 32), 0)[0]) - 1 == 1856
    xy = nb.world_tables(nb.step_bank(), 2)[0]
    assert (len(xy) - 1 + nb.CHUNK - 1) // nb.CHUNK > 256                      # the route for paths of more than 256 chunks
    assert [len(nb.world_tables(nb.straight_path(n), 0)[0]) - 1 for n in nb.STRAIGHT_SIZES] == [1, 63, 64, 65, 128, 129]
    assert [len(nb.world_tables(b(), 0)[2]) for b in (nb.knots_two, nb.knots_three)] == [2, 3]


@pytest.mark.parametrize("name", nb.CASE_NAMES)
def test_oracle_agrees_with_brute_force(name):
    """s and the navigation columns to 1e-12; the chosen segment is checked through the BITS of the arclength (the oracle keeps no
    segment index), not through the index itself."""
    c = nb.case(name)
    assert len(c.poses) <= 64
    ora = nb.oracle_nav(c)
    info, nav = ora.read("INFO64"), ora.read("NAV64")
    want = nb.brute_force_rows(c)
    np.testing.assert_allclose(info[:, 6], want[:, 0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(nav[:, nb.NAV_COLS], want[:, 1:], rtol=0, atol=1e-12)
    # the chosen segment, exactly: the oracle keeps no index, but its arclength is formed from the chosen segment alone -- on
    # these dyadic tables without rounding, so the same bits <=> the same segment (or a repeated vertex's twin)
    np.testing.assert_array_equal(info[:, 6], want[:, 0])
    ora.close()


def test_oracle_agrees_with_brute_force_on_the_step_batch():
    bank = nb.step_bank()
    ties = nb.step_tie_poses()
    c = nb.Case("step", bank, np.array([[x, y, 0.0] for _, x, y in ties]), np.array([w for w, _, _ in ties], dtype=np.int32), (), (), (), 300)
    ora = nb.oracle_nav(c)
    np.testing.assert_array_equal(ora.read("INFO64")[:, 6], nb.brute_force_rows(c)[:, 0])
    for w, x, y in ties:
        js, ss = nb.tied_segments(bank, w, x, y)
        assert len(js) >= 2 and ss.max() - ss.min() > 50.0, (w, x, y)
    ora.close()


@pytest.mark.parametrize("name", ["u32", "u8", "comb"])
def test_far_tie_poses_tie_exactly(name):
    c = nb.case(name)
    assert len(c.far_tie) >= 6
    for i in c.far_tie:
        x, y, _ = c.poses[i]
        js, ss = nb.tied_segments(c.bank, int(c.world[i]), x, y)               # bit-equal distances
        assert len(js) >= 2 and ss.max() - ss.min() > 50.0, (name, i, js, ss)
        assert nb.brute_force_nav(c.bank, int(c.world[i]), x, y)[1] == ss.min()


@pytest.mark.parametrize("name", ["u32", "u8", "comb"])
def test_memory_route_poses_keep_three_chunks(name):
    c = nb.case(name)
    assert len(c.memory) >= 4
    for i, h in c.memory:
        x, y, _ = c.poses[i]
        w = int(c.world[i])
        tied, within_u = nb.chunks_sure_to_survive(c.bank, w, x, y, nb.hint_value(c.bank, w, x, y, h))
        assert tied >= 3 or within_u >= 3, (name, i, h, tied, within_u)


def test_routes_covered():
    """Coverage (a model of the pruning, see circle_model_survivors): some tie is settled between the two chunks held in
    registers, some survivor list is odd (a last trip to memory with one chunk), some even."""
    counts = {}
    for name in ("u32", "u8", "comb"):
        c = nb.case(name)
        for i in c.far_tie:
            x, y, _ = c.poses[i]
            for h in nb.HINTS:
                counts[name, i, h] = nb.circle_model_survivors(c.bank, 0, x, y, nb.hint_value(c.bank, 0, x, y, h))
    assert sum(v == 2 for v in counts.values()) >= 6
    assert any(v is not None and v > 2 and v % 2 == 1 for v in counts.values())
    assert any(v is not None and v > 2 and v % 2 == 0 for v in counts.values())


@pytest.mark.parametrize("name", ["knots8", "knots300"])
def test_walk_queries_miss_the_uniform_guess(name):
    c = nb.case(name)
    assert len(c.walk) >= 12
    up = down = 0
    for i in c.walk:
        _, _, knot_s, _, L = nb.world_tables(c.bank, int(c.world[i]))
        s = nb.brute_force_nav(c.bank, int(c.world[i]), c.poses[i][0], c.poses[i][1])[1]
        guess = int(s / L * (len(knot_s) - 1))
        true = int(np.searchsorted(knot_s, s, side="right") - 1)
        assert abs(guess - true) >= 3, (i, s, guess, true)
        up, down = up + (true > guess), down + (true < guess)
    assert up >= 4 and down >= 4                                              # the walk runs both ways


@pytest.mark.parametrize("name", ["knots8", "knots300"])
def test_knot_cases_hold_what_they_name(name):
    c = nb.case(name)
    on_knot = clipped = exact_L = 0
    for w, (x, y, _) in zip(c.world, c.poses):
        _, _, knot_s, _, L = nb.world_tables(c.bank, int(w))
        s = nb.brute_force_nav(c.bank, int(w), x, y)[1]
        on_knot += s in knot_s
        clipped += s + c.look_ahead > L
        exact_L += s + c.look_ahead == L
    assert on_knot >= 10 and clipped >= 10 and (exact_L >= 1 or c.look_ahead != 8)
