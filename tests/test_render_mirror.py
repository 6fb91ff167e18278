"""CPU: the NumPy mirror of the renderer's pixel rule (gym_auv_amd/render.py) on hand-made geometry -- exact pixel counts by the
even-odd rule, the `<=` of the line rule on pixel-centre boundaries, the layer order, the beam colour formula, the NaN-terminated
trail -- and the argument checks BatchedAuvEnv.render makes before anything reaches the library."""
import numpy as np
import pytest

from gym_auv_amd import render as R

PAL = R.DEFAULT_PALETTE
H, W = 16, 24


def _frame(zoom=1.0, path=None, shapes=(), dyn=None, rays=None, q=None, trail=None, markers=None, line_px=1.0, x=0.0, y=0.0):
    """One north-up frame centred on (x, y): pixel (i, j) has its centre at (x + (j + 0.5 - W / 2) / zoom, y - (i + 0.5 - H / 2) / zoom)."""
    cam = np.array([[x, y, 1.0 / zoom, 0.0, 0.0, -1.0 / zoom, zoom, 1.0]])
    dyn = np.zeros((1, 10, 4)) if dyn is None else dyn
    rays = np.zeros((1, 1, 4)) + 1e9 if rays is None else rays
    q = np.zeros((1, rays.shape[1]), dtype=np.uint8) if q is None else q
    tab = R.WorldTables(np.zeros((0, 2)) if path is None else np.asarray(path, dtype=np.float64), list(shapes))
    return R.render_reference(cam, dyn, rays, q, [tab], trail, markers, None, H, W, line_px)[0]


def _is(frame, layer):
    return (frame == PAL[layer]).all(axis=2)


def _square(x0, y0, side):
    p = np.array([[x0, y0], [x0 + side, y0], [x0 + side, y0 + side], [x0, y0 + side]], dtype=np.float64)
    return np.concatenate([p, np.roll(p, -1, axis=0)], axis=1)


def test_square_obstacle_pixel_counts_at_zoom_1_and_2():
    # pixel centres sit on half-integers: a 4 m square with integer corners holds exactly 4 x 4 of them at zoom 1, 8 x 8 at zoom 2
    for zoom, n in ((1.0, 16), (2.0, 64)):
        f = _frame(zoom=zoom, shapes=[_square(-2.0, -1.0, 4.0)])
        assert _is(f, R.OBSTACLE).sum() == n and _is(f, R.BG).sum() == H * W - n
    # edges ON pixel centres: a centre on the left / lower edge is inside, one on the right / upper edge is not (half-open rule)
    f = _frame(shapes=[_square(-1.5, -1.5, 3.0)])
    assert _is(f, R.OBSTACLE).sum() == 9
    rows, cols = np.nonzero(_is(f, R.OBSTACLE))
    assert cols.min() == W // 2 - 2 and cols.max() == W // 2 and rows.min() == H // 2 - 1 and rows.max() == H // 2 + 1


def test_two_overlapping_shapes_do_not_cancel():
    f = _frame(shapes=[_square(-2.0, -2.0, 4.0), _square(-1.0, -1.0, 4.0)])
    assert _is(f, R.OBSTACLE).sum() == 16 + 16 - 9


def test_horizontal_line_of_one_pixel_lights_one_row_and_the_boundary_follows_le():
    f = _frame(path=[[-100.0, 0.5], [100.0, 0.5]])                   # through the centres of one row
    lit = _is(f, R.PATH)
    assert lit.sum() == W and lit[H // 2 - 1].all()
    f = _frame(path=[[-100.0, 0.0], [100.0, 0.0]])                   # midway between two rows: both are exactly h = 0.5 away
    lit = _is(f, R.PATH)
    assert lit.sum() == 2 * W and lit[H // 2 - 1].all() and lit[H // 2].all()
    f = _frame(path=[[-100.0, 0.25], [100.0, 0.25]])                 # 0.25 from one row, 0.75 from the other
    assert _is(f, R.PATH).sum() == W
    f = _frame(path=[[-100.0, 0.5], [100.0, 0.5]], line_px=3.0)      # h = 1.5: the row and both neighbours (|d| = 1 <= 1.5)
    assert _is(f, R.PATH).sum() == 3 * W
    f = _frame(path=[[0.5, 0.5], [0.5, 0.5]])                        # a degenerate segment is a dot of radius h
    assert _is(f, R.PATH).sum() == 1


def test_layer_order():
    sq = _square(-3.0, -3.0, 6.0)
    path = [[-100.0, 0.5], [100.0, 0.5]]
    trail = np.array([[[0.5, -100.0], [0.5, 100.0]]])
    markers = np.array([[[0.5, 0.5, 1.2]]])
    dyn = np.zeros((1, 10, 4))
    dyn[0, 0:4], dyn[0, 4] = _square(-1.0, -1.0, 2.0), 0.0           # a "mover" (four edges and a null one)
    f = _frame(path=path, trail=trail, shapes=[sq], markers=markers, dyn=dyn)
    c = (H // 2 - 1, W // 2)                                          # the pixel centred on (0.5, 0.5)
    assert (f[c] == PAL[R.MOVER]).all()
    assert (f[c[0], W // 2 + 5] == PAL[R.PATH]).all() and (f[c[0], W // 2 + 2] == PAL[R.OBSTACLE]).all()
    assert (f[0, W // 2] == PAL[R.TRAIL]).all()                       # the trail crosses the path outside the obstacle ...
    f2 = _frame(path=path, trail=trail)
    assert (f2[c] == PAL[R.TRAIL]).all()                              # ... and lies over it where they cross
    dyn[0, 5:9] = _square(0.0, 0.0, 1.0)                              # the vessel over everything, the beams over the mover
    rays = np.array([[[0.5, 0.5, 0.5, 0.5], [0.5, 0.5, 1.5, 0.5]]])
    f3 = _frame(shapes=[sq], markers=markers, dyn=dyn, rays=rays, q=np.array([[0, 255]], dtype=np.uint8))
    assert (f3[c] == PAL[R.VESSEL]).all()
    assert (f3[c[0], c[1] + 1] == PAL[R.RAY_HI]).all()                # only beam 1 reaches the next pixel
    dyn[0, 5:9] = 0.0
    f4 = _frame(shapes=[sq], markers=markers, dyn=dyn, rays=rays, q=np.array([[0, 255]], dtype=np.uint8))
    assert (f4[c] == PAL[R.RAY_HI]).all()                             # both beams light the centre pixel: the higher index wins
    f5 = _frame(shapes=[sq], markers=markers, dyn=np.zeros((1, 10, 4)))
    assert (f5[c] == PAL[R.MARKER]).all()                             # marker over obstacle


@pytest.mark.parametrize("q", [0, 128, 255])
def test_beam_colour_formula(q):
    rays = np.array([[[-100.0, 0.5, 100.0, 0.5]]])
    f = _frame(rays=rays, q=np.array([[q]], dtype=np.uint8))
    lo, hi = PAL[R.RAY_LO].astype(int), PAL[R.RAY_HI].astype(int)
    want = (lo * (255 - q) + hi * q + 127) // 255
    assert (f[H // 2 - 1] == want).all() and (f[H // 2] == PAL[R.BG]).all()
    if q == 0:
        assert (want == lo).all()
    if q == 255:
        assert (want == hi).all()


def test_nan_row_ends_the_trail():
    trail = np.array([[[-100.0, 0.5], [100.0, 0.5], [np.nan, np.nan], [0.5, -100.0], [0.5, 100.0]]])
    f = _frame(trail=trail)
    assert _is(f, R.TRAIL).sum() == W                                 # the vertical stretch behind the NaN row is not drawn
    trail[0, 2] = [100.0, 0.5]
    assert _is(_frame(trail=trail), R.TRAIL).sum() == W + H - 1                # (the row, the column, one pixel shared)
    trail[0, 0, 1] = np.nan                                           # a NaN in the first row: no trail at all
    assert _is(_frame(trail=trail), R.TRAIL).sum() == 0
    assert R.trail_rows(np.zeros((3, 2))) == 3


def test_tiling_and_ppm(tmp_path):
    frames = np.arange(5 * 2 * 3 * 3, dtype=np.uint8).reshape(5, 2, 3, 3)
    big = R.tile_frames(frames)
    assert big.shape == (4, 9, 3) and (big[0:2, 3:6] == frames[1]).all() and (big[2:4, 3:6] == frames[4]).all() and (big[2:4, 6:9] == 0).all()
    R.write_ppm(str(tmp_path / "a.ppm"), frames[0])
    blob = open(tmp_path / "a.ppm", "rb").read()
    assert blob == b"P6\n3 2\n255\n" + frames[0].tobytes()


def test_argument_checks():
    ok = dict(n_envs=8, envs=[0, 7, 0], size=(600, 720), zoom=1.5, view="heading_up")
    assert R.check_render_args(**ok).tolist() == [0, 7, 0]
    assert R.check_render_args(**dict(ok, envs=None)).tolist() == list(range(8))
    assert len(R.check_render_args(**dict(ok, n_envs=4096, envs=None))) == 16
    for bad in (dict(envs=[]), dict(size=(0, 10)), dict(size=(10, 0)), dict(size=(4097, 10)), dict(size=(10, 4097)), dict(envs=[8]),
                dict(envs=[-1]), dict(zoom=0.0), dict(zoom=-2.0), dict(zoom=float("nan")), dict(zoom=float("inf")),
                dict(view="sideways"), dict(line_px=0.0), dict(envs=[0.5])):
        with pytest.raises(ValueError):
            R.check_render_args(**dict(ok, **bad))
    with pytest.raises(ValueError):
        R.check_palette(np.zeros((8, 3), dtype=np.uint8))
    assert R.check_palette(None) is R.DEFAULT_PALETTE
