"""Numpy restatement of the device cloud sampler (csrc/gwtf_clouds.hip), shared by test_clouds_cpu.py and test_gpu_clouds.py:
Philox4x32-10, the draws of one call, the reference's face search in float64 and its float32 point arithmetic."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two -> four uint32 arrays (Random123 philox4x32, 10 rounds)."""
    c = [np.asarray(x, np.uint64) & MASK for x in np.broadcast_arrays(*counter)]
    k = [np.uint64(int(key[0]) & 0xffffffff), np.uint64(int(key[1]) & 0xffffffff)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return [x.astype(np.uint32) for x in c]


def draws(seed, call, B, M, stream=0):
    """The four words of every (row, point) of one call: each (B, M) uint32."""
    j, r = np.meshgrid(np.arange(M, dtype=np.uint64), np.arange(B, dtype=np.uint64))
    seed, call = int(seed) & (2**64 - 1), int(call)
    return philox4x32_10((j, r, call & 0xffffffff, (call >> 32) | (stream << 28)), (seed & 0xffffffff, seed >> 32))


def sampling_draws(seed, call, B, M):
    """(face words uint32, s1, s2 float32), each (B, M): stream 0."""
    w = draws(seed, call, B, M, 0)
    return w[0], (w[1] >> 8).astype(np.float32) * np.float32(2.0**-24), (w[2] >> 8).astype(np.float32) * np.float32(2.0**-24)


def noise_draws(seed, call, B, M):
    """(B, 3, M) float32 standard normals: stream 1, Box-Muller on (w0, w1) -> x, y and (w2, w3) -> z."""
    w = draws(seed, call, B, M, 1)

    def pair(a, b):
        u1 = ((a >> 8).astype(np.float32) + np.float32(1)) * np.float32(2.0**-24)
        u2 = (b >> 8).astype(np.float32) * np.float32(2.0**-24)
        rad, ang = np.sqrt(np.float32(-2) * np.log(u1)), np.float32(2 * np.pi) * u2
        return rad * np.cos(ang), rad * np.sin(ang)
    x, y = pair(w[0], w[1])
    z, _ = pair(w[2], w[3])
    return np.stack([x, y, z], axis=1).astype(np.float32)


def reference_cdf(vertices, faces):
    """sample_cloud's float32 areas and probabilities and RandomState.choice's float64 CDF."""
    polygons = vertices[faces.astype(np.int64)]
    cross = np.cross(polygons[:, 2] - polygons[:, 0], polygons[:, 2] - polygons[:, 1])
    areas = np.sqrt((cross**2).sum(1)) / 2.0
    probs = areas / areas.sum()
    assert areas.dtype == np.float32 and probs.dtype == np.float32
    cdf = np.cumsum(probs.astype(np.float64))
    cdf /= cdf[-1]
    return areas, probs, cdf


def shape_arrays(packed, shape):
    vertices_c, faces_vc, vb, fb = packed
    return (np.asarray(vertices_c, np.float32)[int(vb[shape]):int(vb[shape + 1])],
            np.asarray(faces_vc)[int(fb[shape]):int(fb[shape + 1])].astype(np.int64))


def restate(packed, rows, words, s1, s2):
    """(faces (B, M), points (B, 3, M) float32): searchsorted(cdf, w * 2^-32, 'right') and the reference's point arithmetic."""
    B, M = words.shape
    faces = np.zeros((B, M), np.int64)
    points = np.zeros((B, 3, M), np.float32)
    for r, shape in enumerate(rows):
        v, f = shape_arrays(packed, int(shape))
        cdf = reference_cdf(v, f)[2]
        faces[r] = np.searchsorted(cdf, words[r].astype(np.float64) * 2.0**-32, side='right')
        a1, a2 = s1[r][:, None].astype(np.float32).copy(), s2[r][:, None].astype(np.float32).copy()
        cond = (a1 + a2) > 1.
        a1[cond] = 1. - a1[cond]
        a2[cond] = 1. - a2[cond]
        sp = v[f][faces[r]]
        p = sp[:, 0] + a1 * (sp[:, 1] - sp[:, 0]) + a2 * (sp[:, 2] - sp[:, 0])
        assert p.dtype == np.float32
        points[r] = p.T
    return faces, points


def random_mesh(n_faces, n_vertices, seed, leading_zero_area=False):
    rng = np.random.RandomState(seed)
    v = rng.uniform(-0.5, 0.5, (n_vertices, 3)).astype(np.float32)
    f = np.stack([rng.choice(n_vertices, 3, replace=False) for _ in range(n_faces)]).astype(np.uint32)
    if leading_zero_area:
        f[0, 1] = f[0, 0]
    return v, f


def pack(meshes):
    """[(vertices, faces)] -> the four packed arrays of meshes.h5."""
    return (np.concatenate([v for v, _ in meshes]).astype(np.float32), np.concatenate([f for _, f in meshes]).astype(np.uint32),
            np.cumsum([0] + [len(v) for v, _ in meshes]).astype(np.uint64),
            np.cumsum([0] + [len(f) for _, f in meshes]).astype(np.uint64))
