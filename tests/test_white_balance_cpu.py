"""Auto white balance without a GPU: argument validation, the C entry points' host checks, the NumPy restatement of the
contract (tests/awb_ref.py) pinned by hand-derived vectors, and a gloo two-rank run of the update's control flow."""
import ctypes
import dataclasses
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from taichi_image_amd import camera_isp
from taichi_image_amd.white_balance import AutoWhiteBalance, check_auto_white_balance, check_seed
from tests import awb_ref as A

f32 = np.float32
Q = 2 ** 24                                    # the fixed-point scale of the statistics


def flat(H, W, site_values):
    """An H x W frame of pre-cast values, site s = (row & 1) * 2 + (col & 1) holding site_values[s]."""
    x = np.empty((H, W), f32)
    for s, v in enumerate(site_values):
        x[s >> 1::2, s & 1::2] = f32(v)
    return x


def by_colour(pattern, r, g, b):
    """Site values of a frame whose red, green and blue pixels hold r, g, b under `pattern`."""
    return [(r, g, b)[c] for c in A.SITE_COLOUR[pattern]]


# ---- argument validation ---------------------------------------------------------------------------------------------
def test_auto_white_balance_settings():
    assert AutoWhiteBalance() == AutoWhiteBalance(4, 0.95, 0.02)
    assert check_auto_white_balance(False) is None
    assert check_auto_white_balance(True) == AutoWhiteBalance()
    cfg = AutoWhiteBalance(stride=2, clip=0.9, floor=0.1)
    assert check_auto_white_balance(cfg) is cfg
    for bad in (dict(stride=0), dict(stride=1.5), dict(stride=True), dict(clip=float("inf")), dict(floor=float("nan")),
                dict(floor=0.0), dict(floor=0.5, clip=0.5), dict(floor=0.6, clip=0.5), dict(clip="1")):
        with pytest.raises(ValueError):
            AutoWhiteBalance(**bad)
    for bad in (None, 1, "on", 0.5):
        with pytest.raises(ValueError):
            check_auto_white_balance(bad)
    with pytest.raises(dataclasses.FrozenInstanceError):
        cfg.stride = 3


def test_seed_validation():
    assert check_seed(np.array([1.8, 1.0, 2.1])).dtype == np.float32
    for bad in (np.array([1.0, 0.0, 1.0]), np.array([1.0, -1.0, 1.0]), np.array([1.0, np.nan, 1.0]),
                np.array([1.0, np.inf, 1.0]), np.array([1.0, 1.0])):
        with pytest.raises(ValueError):
            check_seed(bad)


def test_camera_rejects_bad_settings_before_any_device_work():
    for kw in (dict(auto_white_balance="yes"), dict(auto_white_balance=1),
               dict(auto_white_balance=True, white_balance=np.array([1.0, 0.0, 2.0])),
               dict(auto_white_balance=AutoWhiteBalance(), white_balance=np.array([np.nan, 1.0, 2.0]))):
        with pytest.raises(ValueError):
            camera_isp.Camera16(camera_isp.bayer.BayerPattern.RGGB, **kw)
    # an ISP without AWB keeps today's colour matrix and takes no AWB state
    isp = camera_isp.Camera32(camera_isp.bayer.BayerPattern.RGGB, correct_colors=True)
    assert isp.auto_white_balance is None and isp.white_balance_gains is None
    want = camera_isp.default_cc.copy()
    want[:, :3] *= np.array([1.8, 1.0, 2.1])
    assert np.array_equal(isp.color_correct_matrix, want)
    isp.update_white_balance()                                   # a no-op with AWB off
    for kw in (dict(auto_white_balance="x"), dict(auto_white_balance=True, white_balance=np.array([1.0, 1.0, -2.0]))):
        with pytest.raises(ValueError):
            isp.set(**kw)
        assert isp.auto_white_balance is None
    assert np.array_equal(isp.white_balance, np.array([1.8, 1.0, 2.1]))


# ---- the C entry points reject bad arguments on the host -------------------------------------------------------------
def test_awb_entry_points_validate_on_the_host():
    from taichi_image_amd import _native
    L = _native.lib()
    assert L.mi_isp_version() >= 1600
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    one = (ctypes.c_void_p * 1)(p)

    def packed(**kw):
        a = dict(frames=one, n=1, H=4, W=8, bits=12, ids=0, lv=None, sh=None, clip=0.95, floor=0.02, stride=4, pend=p)
        a.update(kw)
        return L.mi_isp_awb_stats_packed(a["frames"], a["n"], a["H"], a["W"], a["bits"], a["ids"], a["lv"], a["sh"],
                                         a["clip"], a["floor"], a["stride"], a["pend"], None)

    for kw, word in ((dict(bits=10), b"bits"), (dict(H=3), b"even"), (dict(stride=0), b"stride"),
                     (dict(floor=0.0), b"floor"), (dict(floor=0.95), b"floor"), (dict(clip=float("nan")), b"floor"),
                     (dict(pend=None), b"pending"), (dict(n=-1), b"negative"),
                     (dict(frames=(ctypes.c_void_p * 1)(None)), b"null"),
                     (dict(lv=_native.levels_arg([0, 0, 0, 4095], 4095)), b"level"),
                     (dict(lv=_native.levels_arg([0] * 4, 4096)), b"level"),
                     (dict(sh=_native.Shading(p.value, 3, 4, 4)), b"sites"),
                     (dict(sh=_native.Shading(p.value, 1, 1, 4)), b"grid"),
                     (dict(sh=_native.Shading(None, 1, 4, 4)), b"gains")):
        assert packed(**kw) != 0, kw
        assert word in L.mi_isp_last_error(), (kw, L.mi_isp_last_error())
        assert b"awb" in L.mi_isp_last_error()

    def cfa(**kw):
        a = dict(src=p, H=4, W=8, mode=0, lv=None, sh=None, clip=0.95, floor=0.02, stride=4, pend=p)
        a.update(kw)
        return L.mi_isp_awb_stats_cfa(a["src"], a["H"], a["W"], a["mode"], a["lv"], a["sh"], a["clip"], a["floor"],
                                      a["stride"], a["pend"], None)

    for kw, word in ((dict(src=None), b"null"), (dict(mode=3), b"mode"), (dict(stride=-2), b"stride"),
                     (dict(floor=1.0, clip=0.5), b"floor"), (dict(pend=None), b"pending"),
                     (dict(mode=1, lv=_native.levels_arg([0] * 4, 100)), b"u16"),
                     (dict(lv=_native.levels_arg([0] * 4, 70000)), b"level"),
                     (dict(sh=_native.Shading(p.value, 2, 4, 4)), b"sites")):
        assert cfa(**kw) != 0, kw
        assert word in L.mi_isp_last_error(), (kw, L.mi_isp_last_error())

    def update(**kw):
        a = dict(g=p, world=1, pend=p, pattern=0, t=0.9, state=p, gains=p, user=None, E=p)
        a.update(kw)
        return L.mi_isp_awb_update(a["g"], a["world"], a["pend"], a["pattern"], a["t"], a["state"], a["gains"], a["user"],
                                   a["E"], None)

    for kw, word in ((dict(g=None), b"null"), (dict(state=None), b"null"), (dict(gains=None), b"null"),
                     (dict(pend=None), b"null"), (dict(world=0), b"world"), (dict(pattern=4), b"pattern"),
                     (dict(t=float("inf")), b"finite"), (dict(E=None), b"effective"),
                     (dict(user=_native.Shading(p.value, 4, 65, 4)), b"grid")):
        assert update(**kw) != 0, kw
        assert word in L.mi_isp_last_error(), (kw, L.mi_isp_last_error())
    assert L.mi_isp_awb_rebuild(0, None, None, p, None) != 0 and b"gains" in L.mi_isp_last_error()
    assert L.mi_isp_awb_rebuild(-1, p, None, p, None) != 0 and b"pattern" in L.mi_isp_last_error()
    assert L.mi_isp_awb_rebuild(0, p, None, None, None) != 0 and b"effective" in L.mi_isp_last_error()


# ---- the contract, by hand ---------------------------------------------------------------------------------------------
def test_flat_frame_with_a_cast_gives_exact_gains():
    x = flat(8, 8, [0.5, 0.25, 0.25, 0.125])                    # RGGB: R 0.5, G 0.25, B 0.125
    P = A.stats(x, stride=1)
    assert P == [16 * Q // 2, 16 * Q // 4, 16 * Q // 4, 16 * Q // 8, 16]
    st = A.State([1.8, 1.0, 2.1]).update(P, 0, 0.1)
    assert st.S == [0.5, 0.25, 0.125]
    assert st.gains.tolist() == [0.5, 1.0, 2.0]
    # the default stride 4 samples quads (0, 0), (0, 4), (4, 0), (4, 4) of a 16 x 16 frame
    assert A.stats(flat(16, 16, [0.5, 0.25, 0.25, 0.125]))[4] == 4
    assert A.stats(flat(18, 18, [0.5, 0.25, 0.25, 0.125]))[4] == 9      # quads 0, 4, 8 of 9 per axis
    # the user's gains scale the sums, not the filter: a gain of 2 on a 0.6 value still passes the clip
    g = np.full((8, 8), 2.0, f32)
    assert A.stats(flat(8, 8, [0.6, 0.3, 0.3, 0.15]), g, stride=1) == A.stats(flat(8, 8, [1.2, 0.6, 0.6, 0.3]), clip=2.0,
                                                                              stride=1)


def test_fixed_point_rounding():
    x = flat(2, 2, [f32(1) / f32(3), 0.5, 0.5, 0.5])
    P = A.stats(x, stride=1)
    assert P[0] == int(np.rint(f32(f32(1) / f32(3)) * f32(Q)))                  # rint of the f32 product
    xs = flat(2, 2, [0.5, 0.5, 0.5, 0.5])
    assert A.stats(xs, np.full((2, 2), 16.0, f32), stride=1)[0] == 8 * Q      # 0.5 * 16 = 8, within the 2^15 cap
    assert A.stats(flat(2, 2, [0.5, -0.25, 0.5, 0.5]), stride=1)[1] == 0       # negative values count as 0


def test_saturated_and_dark_quads_are_dropped():
    x = flat(8, 8, [0.5, 0.25, 0.25, 0.125])
    x[0, 1] = f32(0.96)                                          # quad (0, 0): one value above the clip
    x[2, 2] = f32(0.95)                                          # quad (1, 1): exactly at the clip (x < clip fails)
    x[4:6, 4:6] = f32(0.01)                                      # quad (2, 2): every value below the floor
    x[6:8, 0:2] = f32(0.01)
    x[7, 1] = f32(0.02)                                          # quad (3, 0): max exactly at the floor: kept
    x[0, 6] = np.nan                                             # quad (0, 3): a NaN
    P = A.stats(x, stride=1)
    assert P[4] == 16 - 4
    assert P[3] == (16 - 5) * Q // 8 + int(np.rint(f32(0.02) * f32(Q)))
    assert A.stats(x, stride=1, clip=0.97)[4] == 16 - 2           # the clip moved: quads (0, 0) and (1, 1) return


def test_no_quad_keeps_the_state():
    st = A.State([1.8, 1.0, 2.1])
    assert st.update([0, 0, 0, 0, 0], 0, 0.1).gains.tolist() == [f32(1.8), 1.0, f32(2.1)] and not st.valid
    st.update(A.stats(flat(8, 8, [0.5, 0.25, 0.25, 0.125]), stride=1), 0, 0.1)
    before = (list(st.S), st.gains.copy())
    st.update(A.stats(flat(8, 8, [0.01] * 4), stride=1), 0, 0.1)            # nothing kept
    assert st.S == before[0] and np.array_equal(st.gains, before[1])


@pytest.mark.parametrize("pattern", [0, 1, 2, 3])
def test_every_pattern_maps_sites_to_colours(pattern):
    x = flat(8, 8, by_colour(pattern, 0.5, 0.25, 0.125))
    st = A.State([1.0, 1.0, 1.0]).update(A.stats(x, stride=1), pattern, 0.1)
    assert st.gains.tolist() == [0.5, 1.0, 2.0]
    # the two greens are averaged: 0.1875 and 0.3125 give G = 0.25 wherever they sit
    vals = by_colour(pattern, 0.5, 0.25, 0.125)
    greens = [s for s in range(4) if A.SITE_COLOUR[pattern][s] == 1]
    vals[greens[0]], vals[greens[1]] = 0.1875, 0.3125
    assert A.State([1.0] * 3).update(A.stats(flat(8, 8, vals), stride=1), pattern, 0.1).S == [0.5, 0.25, 0.125]
    # E: each site carries its colour's gain
    E = A.effective(st.gains, pattern)
    for s in range(4):
        assert (E[s] == [0.5, 1.0, 2.0][A.SITE_COLOUR[pattern][s]]).all()


def test_gains_clamp_to_an_eighth_and_eight():
    x = flat(8, 8, [0.03125, 0.5, 0.5, 0.875])                  # RGGB: G / R = 16, G / B = 4 / 7
    assert A.State([1.0] * 3).update(A.stats(x, stride=1), 0, 0.1).gains.tolist() == [8.0, 1.0, f32(4 / 7)]
    x = flat(8, 8, [0.875, 0.0625, 0.0625, 0.03125])            # G / R = 1 / 14, G / B = 2
    assert A.State([1.0] * 3).update(A.stats(x, stride=1), 0, 0.1).gains.tolist() == [0.125, 1.0, 2.0]
    x = flat(8, 8, [0.0, 0.5, 0.5, 0.5])                        # S_R = 0: g_R keeps its previous value
    assert A.State([1.5, 2.0, 3.0]).update(A.stats(x, stride=1), 0, 0.1).gains.tolist() == [1.5, 1.0, 1.0]


def test_lerp_sequence_starts_with_t_zero():
    st = A.State([1.8, 1.0, 2.1])
    frames = [[0.5, 0.25, 0.25, 0.125], [0.25, 0.25, 0.25, 0.25], [0.125, 0.5, 0.5, 0.5]]
    S = None
    for k, v in enumerate(frames):
        st.update(A.stats(flat(8, 8, v), stride=1), 0, 0.25)
        c = [v[0], v[1], v[3]]
        S = list(c) if k == 0 else [c[i] + 0.75 * (S[i] - c[i]) for i in range(3)]
        assert st.S == S
        assert st.gains.tolist() == [f32(min(max(S[1] / S[0], 0.125), 8)), 1.0, f32(min(max(S[1] / S[2], 0.125), 8))]
    assert st.S[0] == 0.125 + 0.75 * ((0.25 + 0.75 * (0.5 - 0.25)) - 0.125)


def test_effective_grid_of_a_user_grid():
    rng = np.random.default_rng(3)
    g = np.array([0.7, 1.0, 1.3], f32)
    U1 = rng.uniform(1, 2, (5, 7)).astype(f32)
    E = A.effective(g, 2, U1)                                    # GBRG: sites G B R G
    assert E.shape == (4, 5, 7) and E.dtype == f32
    assert np.array_equal(E[1], U1 * g[2]) and np.array_equal(E[2], U1 * g[0]) and np.array_equal(E[3], U1)
    U4 = rng.uniform(1, 2, (4, 3, 3)).astype(f32)
    E = A.effective(g, 0, U4)
    assert np.array_equal(E[0], U4[0] * g[0]) and np.array_equal(E[3], U4[3] * g[2])
    assert A.effective(g, 0).shape == (4, 2, 2)


# ---- two ranks (gloo): the pending rows all-gathered, summed and updated as one ------------------------------------------
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _frames():
    rng = np.random.default_rng(11)
    return [rng.uniform(0.0, 1.0, (32, 48)).astype(f32) * f32(0.5 + 0.1 * i) for i in range(6)]


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from taichi_image_amd import distributed as D
    frames = _frames()[rank::world]
    st = A.State([1.8, 1.0, 2.1])
    out = []
    for step in range(3):
        mine = A.add(*[A.stats(f * f32(1 + 0.2 * step), stride=2) for f in frames])
        gathered = D.all_gather_rows(torch.tensor(mine, dtype=torch.int64), dist.group.WORLD)
        assert gathered.shape == (world, 5) and gathered.dtype == torch.int64
        st.update(A.add(*gathered.tolist()), 1, 0.3)
        out.append((list(st.S), st.gains.tolist()))
    q.put((rank, out))
    dist.destroy_process_group()


def test_two_ranks_match_one_process():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    st = A.State([1.8, 1.0, 2.1])
    want = []
    for step in range(3):
        st.update(A.add(*[A.stats(f * f32(1 + 0.2 * step), stride=2) for f in _frames()]), 1, 0.3)
        want.append((list(st.S), st.gains.tolist()))
    assert got[0] == want and got[1] == want
