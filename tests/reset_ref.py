"""
CPU restatement of the in-place reset's placement (swarm_reset.cuh:
k_place_envs; DESIGN.md section 3 "Reset placement"), in numpy: Philox4x32-10
written out here, fp32 arithmetic one rounding per operation, and the
oracle's sincos_turn for the one polynomial.  TEST INFRASTRUCTURE ONLY.
"""

import ctypes

import numpy as np

from oracle import oracle

RESET_TAG = 0x30
TWO32 = 4294967296.0
F32 = np.float32


def philox4x32_10(ctr, key):
    """ctr: 4 arrays (or scalars) of uint32, key: 2 -> 4 uint32 arrays."""
    c = [np.atleast_1d(np.asarray(v, np.uint64)) & np.uint64(0xFFFFFFFF) for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    m32 = np.uint64(0xFFFFFFFF)
    for r in range(10):
        if r > 0:
            k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
            k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
    return [v.astype(np.uint32) for v in c]


def unit_from_word(w):
    """U = (word >> 8) 2^-24 (exact in fp32)."""
    return (np.asarray(w, np.uint32) >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)


def sincos_turn(a):
    """oracle.sincos_turn over an array of turn words -> (sin, cos) fp32."""
    a = np.atleast_1d(np.asarray(a, np.uint32))
    L = oracle.lib()
    s = np.zeros(a.shape, F32)
    c = np.zeros(a.shape, F32)
    sv, cv = ctypes.c_float(), ctypes.c_float()
    for k, w in enumerate(a.ravel()):
        L.or_sincos_turn(int(w), ctypes.byref(sv), ctypes.byref(cv))
        s.flat[k], c.flat[k] = sv.value, cv.value
    return s, c


def f2i32(v):
    """swarm::f2i32: clamp to +-2147483520, round to nearest even."""
    v = np.clip(np.asarray(v, F32), F32(-2147483520.0), F32(2147483520.0))
    return np.rint(v.astype(np.float64)).astype(np.int64)


def place_axis(cq, cimg, dx, box_a):
    """The centre's coordinate (cq, cimg) moved by the fp32 displacement dx:
    dq = f2i32(dx * fp32(2^32 / L)), carried into the image counter."""
    inv_sx = F32(TWO32 / box_a)
    dq = f2i32(np.asarray(dx, F32) * inv_sx)
    v = (np.int64(cimg) << np.int64(32)) + np.int64(cq) + dq
    return (v & np.int64(0xFFFFFFFF)).astype(np.uint32), (v >> np.int64(32)).astype(np.int32)


def place2_from_words(words, centre, radius, box):
    """2-D: words [4] arrays (one Philox block per particle) -> q [2, n],
    img [2, n], ang [n]."""
    x, y, z, w = words
    rad = F32(radius) * np.maximum(unit_from_word(x), unit_from_word(y))
    sn, cs = sincos_turn(z)
    q = np.zeros((2, len(rad)), np.uint32)
    img = np.zeros((2, len(rad)), np.int32)
    for a, u in enumerate((cs, sn)):
        cq, cimg = oracle.to_fixed(centre[a], box[a])
        q[a], img[a] = place_axis(int(cq), int(cimg), rad * u, box[a])
    return q, img, np.asarray(w, np.uint32).copy()


def place3_from_words(w1, w2, centre, radius, box):
    """3-D: two Philox blocks per particle -> q [3, n], img [3, n], dir [3, n]."""
    rad = F32(radius) * np.maximum(np.maximum(unit_from_word(w1[0]), unit_from_word(w1[1])),
                                   unit_from_word(w1[2]))
    zc = F32(2.0) * unit_from_word(w2[0]) - F32(1.0)
    sxy = np.sqrt(F32(1.0) - zc * zc)
    sn, cs = sincos_turn(w1[3])
    disp = (rad * (sxy * cs), rad * (sxy * sn), rad * zc)
    q = np.zeros((3, len(rad)), np.uint32)
    img = np.zeros((3, len(rad)), np.int32)
    for a in range(3):
        cq, cimg = oracle.to_fixed(centre[a], box[a])
        q[a], img[a] = place_axis(int(cq), int(cimg), disp[a], box[a])
    zd = F32(2.0) * unit_from_word(w2[1]) - F32(1.0)
    sd = np.sqrt(F32(1.0) - zd * zd)
    sn, cs = sincos_turn(w2[2])
    return q, img, np.stack([sd * cs, sd * sn, zd]).astype(F32)


def place_env(box, dims, seed, env, ordinal, home, groups):
    """One env after a placement with this reset ordinal.  home: its home
    state (oracle state dict: q, img [3, N], ang [N], 3-D: dir [3, N]);
    groups: [(first, count, centre, radius)].  A particle outside every group
    and a group of radius 0 stay at home."""
    st = {k: np.array(v, copy=True) for k, v in home.items()}
    key = (seed & 0xFFFFFFFF, ((seed >> 32) ^ env) & 0xFFFFFFFF)
    for first, count, centre, radius in groups:
        if count == 0 or radius == 0.0:
            continue
        idx = np.arange(first, first + count, dtype=np.uint32)
        ctr = lambda tag: (idx, ordinal & 0xFFFFFFFF, ordinal >> 32, tag)  # noqa: E731
        sl = slice(first, first + count)
        w1 = philox4x32_10(ctr(RESET_TAG), key)
        if dims == 2:
            q, img, ang = place2_from_words(w1, centre, radius, box)
            st["q"][:2, sl], st["img"][:2, sl], st["ang"][sl] = q, img, ang
        else:
            w2 = philox4x32_10(ctr(RESET_TAG + 1), key)
            q, img, d = place3_from_words(w1, w2, centre, radius, box)
            st["q"][:, sl], st["img"][:, sl], st["dir"][:, sl] = q, img, d
            st["ang"][sl] = 0
    return st
