"""The 3D colour LUT as DESIGN.md 3 ("Colour LUT") states it, in NumPy integers.  It does not call the library: the table is
an (N, N, N, 3) u8 array indexed [r][g][b] and the strength a plain number (S = floor(strength * 64 + 0.5)).  Three switches
give the mutants the tests must tell from the contract; none is the contract.  Also here: the tables and the image the
tests share."""
import math

import numpy as np


def strength_q6(strength):
    return int(math.floor(strength * 64 + 0.5))


def identity_table(N):
    """T[r][g][b] = (q(r), q(g), q(b)), q(k) = (2 * 255 k + (N - 1)) // (2 (N - 1))."""
    q = (2 * 255 * np.arange(N) + (N - 1)) // (2 * (N - 1))
    t = np.empty((N, N, N, 3), np.uint8)
    t[..., 0] = q[:, None, None]
    t[..., 1] = q[None, :, None]
    t[..., 2] = q[None, None, :]
    return t


def random_table(rng, N):
    return rng.integers(0, 256, (N, N, N, 3)).astype(np.uint8)


def look_table(N):
    """A smooth "look": a per-channel curve (three gammas, the red one darker in the cyans), then less saturation, then R and B swapped (so that the axis
    order shows), quantised as ColorLut quantises a float table."""
    k = np.arange(N) / (N - 1)
    r, g, b = np.meshgrid(k, k, k, indexing="ij")
    r, g, b = r ** 0.8 * (1.0 - 0.25 * g * b), g ** 1.1, 0.05 + 0.9 * b ** 1.3  # (the product: no affine map, even at N = 2)
    l = 0.3 * r + 0.6 * g + 0.1 * b
    r, g, b = (l + 0.6 * (c - l) for c in (r, g, b))
    t = np.stack([b, g, r], -1)
    return np.floor(np.clip(t, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def ties_and_ends_image():
    """A (24, 32, 3) image of the cases the sort and the last table point decide: greys (three equal fractions), every
    combination of channels at 0, 255 and two in-between codes, and pixels with exactly two equal channels."""
    px = [(g, g, g) for g in range(0, 256, 5)]
    ends = (0, 255, 1, 254, 77, 200)
    px += [(a, b, c) for a in ends for b in ends for c in ends]
    for u in range(3, 256, 11):
        for v in (0, 40, 128, 255):
            px += [(u, u, v), (u, v, u), (v, u, u)]
    px = np.asarray(px, np.uint8)
    out = np.zeros((24 * 32, 3), np.uint8)
    assert len(px) <= len(out)
    out[:len(px)] = px
    out[len(px):] = px[:len(out) - len(px)]
    return out.reshape(24, 32, 3)


def _interpolate(v, table, reverse_ties, trilinear, truncate, swap_axes):
    """y of the contract for the (P, 3) int64 codes v."""
    N = table.shape[0]
    T = table.astype(np.int64)
    if swap_axes:                                                   # T[b][g][r] (NOT the contract)
        T = T.transpose(2, 1, 0, 3)
    p = v * (N - 1)
    i = p // 255
    f = p - 255 * i
    j = np.minimum(i + 1, N - 1)
    rnd = 0 if truncate else 127                                    # truncate: the + 127 dropped (NOT the contract)
    if trilinear:                                                   # 8 corners, weights in 1 / 255^3 (NOT the contract)
        num = np.zeros((len(v), 3), np.int64)
        for cr in (0, 1):
            for cg in (0, 1):
                for cb in (0, 1):
                    w = np.ones(len(v), np.int64)
                    idx = []
                    for c, bit in enumerate((cr, cg, cb)):
                        w = w * (f[:, c] if bit else 255 - f[:, c])
                        idx.append(j[:, c] if bit else i[:, c])
                    num += T[idx[0], idx[1], idx[2]] * w[:, None]
        return (num + (0 if truncate else 255 ** 3 // 2)) // 255 ** 3
    # the axes ordered so that f_a >= f_b >= f_d; a stable sort either way round, so that ties fall both ways
    if reverse_ties:
        order = 2 - np.argsort(-f[:, ::-1], axis=1, kind="stable")
    else:
        order = np.argsort(-f, axis=1, kind="stable")
    fs = np.take_along_axis(f, order, axis=1)
    assert (fs[:, 0] >= fs[:, 1]).all() and (fs[:, 1] >= fs[:, 2]).all()
    rows = np.arange(len(v))
    corner = i.copy()
    C = [T[corner[:, 0], corner[:, 1], corner[:, 2]]]
    for k in range(3):
        ax = order[:, k]
        corner[rows, ax] = j[rows, ax]
        C.append(T[corner[:, 0], corner[:, 1], corner[:, 2]])
    assert np.array_equal(corner, j)                                # C3 = T[j_R][j_G][j_B]
    w = [255 - fs[:, 0], fs[:, 0] - fs[:, 1], fs[:, 1] - fs[:, 2], fs[:, 2]]
    num = sum(c * wk[:, None] for c, wk in zip(C, w))
    assert num.max(initial=0) <= 65025
    return (num + rnd) // 255


def color_lut_rgb(img, table, strength=1.0, *, trilinear=False, truncate=False, swap_axes=False):
    """The operator on an (H, W, 3) u8 image.  Both orders of tied fractions are computed and must agree."""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    assert table.dtype == np.uint8 and table.ndim == 4 and table.shape[3] == 3 and 2 <= table.shape[0] <= 65
    assert table.shape[0] == table.shape[1] == table.shape[2]
    if img.size == 0:
        return img.copy()
    S = strength_q6(strength)
    assert 0 <= S <= 64
    v = img.reshape(-1, 3).astype(np.int64)
    y = _interpolate(v, table, False, trilinear, truncate, swap_axes)
    if not trilinear:
        assert np.array_equal(y, _interpolate(v, table, True, trilinear, truncate, swap_axes)), "the tie order shows"
    out = v + (((y - v) * S + 32) >> 6)
    assert (out >= np.minimum(v, y)).all() and (out <= np.maximum(v, y)).all()      # between v and y: no clamp
    return out.astype(np.uint8).reshape(img.shape)


# ---- what the GPU tests run, made here so that tests/test_color_lut_cpu.py can show on the CPU that it is not vacuous ------
GPU_POINTS = [2, 3, 17, 33, 34, 65]
GPU_SHAPES = [(1, 1), (1, 5), (3, 7), (5, 4), (31, 33), (64, 64), (70, 131)]
GPU_STRENGTHS = [1.0, 0.5, 1 / 64, 0.0]
_tables = {}


def gpu_tables(N):
    """{name: table} of the GPU tests at N points (fixed seed; made once)."""
    if N not in _tables:
        _tables[N] = {"identity": identity_table(N), "random": random_table(np.random.default_rng(1000 + N), N),
                      "look": look_table(N)}
        for t in _tables[N].values():
            t.setflags(write=False)
    return _tables[N]


def gpu_images(H, W):
    """{name: image} of the GPU tests at H x W (fixed seed): random bytes, the natural scene of sharpen_ref, and the ties
    and ends image (its own shape, whatever H and W are)."""
    from tests import sharpen_ref
    rng = np.random.default_rng(7 * H + W)
    return {"random": rng.integers(0, 256, (H, W, 3)).astype(np.uint8), "scene": sharpen_ref.scene_u8(rng, H, W),
            "ties": ties_and_ends_image()}
