"""Numpy restatement of the device image transform (csrc/gwtf_images.hip), shared by test_images_cpu.py and test_gpu_images.py:
every stage of the reference's ComposeImageTransformation in float32 and in its operation order, the Resize tables in float64, and
the Philox noise of one call (clouds_ref.philox4x32_10); and what both test files share: the config_SVR keys, the fixture's cases and
the Resize bar."""
import json

import numpy as np

import clouds_ref as cr

GRAY = (0.299, 0.587, 0.114)


def to_numpy(image):
    """(C, H, W) uint8 -> float32: byte / 255 (float64 division, rounded), then channels 0 and 1 times channel 2."""
    img = np.float32(image / 255.)
    img[:2] = img[2][None] * img[:2]
    return img


def axis_table(n_src, n_dst):
    """(s, f) of INTER_LINEAR along one axis: the coordinate in float64, rounded to float32 once; f -= s in float32."""
    d = np.arange(n_dst, dtype=np.float64)
    f = np.float32((d + 0.5) * (n_src / n_dst) - 0.5)
    s = np.floor(f).astype(np.int64)
    f = np.float32(f - np.float32(s))
    low, high = s < 0, s >= n_src - 1
    s[low], f[low] = 0, 0
    s[high], f[high] = n_src - 1, 0
    return s, f


def resize(img, size):
    """(C, H, W) float32 -> (C, size[1], size[0]): the horizontal pass, then the vertical one, float32 products and sums."""
    C, H, W = img.shape
    xs, xf = axis_table(W, size[0])
    ys, yf = axis_table(H, size[1])
    x1, y1 = np.minimum(xs + 1, W - 1), np.minimum(ys + 1, H - 1)
    a0, a1 = (np.float32(1) - xf)[None, None, :], xf[None, None, :]
    b0, b1 = (np.float32(1) - yf)[None, :, None], yf[None, :, None]
    rows = img[:, :, xs] * a0 + img[:, :, x1] * a1
    out = rows[:, ys, :] * b0 + rows[:, y1, :] * b1
    assert out.dtype == np.float32
    return out


def pad(img, pad_size):
    out = np.zeros((img.shape[0], img.shape[1] + 2 * pad_size[0], img.shape[2] + 2 * pad_size[1]), np.float32)
    out[:, pad_size[0]:pad_size[0] + img.shape[1], pad_size[1]:pad_size[1] + img.shape[2]] = img
    return out


def add_grayscale(img):
    r, g, b = (np.float32(w) for w in GRAY)
    return np.concatenate([((r * img[0] + g * img[1]) + b * img[2])[None], img])


def normalize(img, means, stds):
    m, s = np.asarray(means, np.float32).reshape(-1, 1, 1), np.asarray(stds, np.float32).reshape(-1, 1, 1)
    return (img - m) / s


def transform_one(image, cfg, noise=None):
    """One (C, H, W) uint8 image through the enabled stages; noise: (C_stage, H_out, W_out) float32, already scaled."""
    img = to_numpy(image)
    if cfg.get('image_resize'):
        img = resize(img, cfg['image_size'])
    if cfg.get('image_pad'):
        img = pad(img, cfg['image_pad_size'])
    if cfg.get('image_add_grayscale'):
        img = add_grayscale(img)
    if cfg.get('image_normalize'):
        img = normalize(img, cfg['image_means'], cfg['image_stds'])
    if cfg.get('image_noise'):
        img = np.minimum(np.maximum(img + noise, np.float32(0)), np.float32(1))
    if cfg.get('image_remove_alpha'):
        img = img[:4]
    assert img.dtype == np.float32
    return img


def transform(images, cfg, noise=None):
    """(B, C, H, W) uint8 -> (B, C_out, H_out, W_out) float32."""
    return np.stack([transform_one(im, cfg, None if noise is None else noise[i]) for i, im in enumerate(images)])


def philox_noise(seed, call, B, C_stage, H_out, W_out, scale):
    """(B, C_stage, H_out, W_out) float32: scale * z, z the Box-Muller normals of the counter (y * W_out + x, b, call): stream 4
    gives (w0, w1) -> channels 0, 1 and (w2, w3) -> channels 2, 3; stream 5 (w0, w1) -> channel 4."""
    def pair(a, b):
        u1 = ((a >> 8).astype(np.float32) + np.float32(1)) * np.float32(2.0**-24)
        u2 = (b >> 8).astype(np.float32) * np.float32(2.0**-24)
        rad, ang = np.sqrt(np.float32(-2) * np.log(u1)), np.float32(2 * np.pi) * u2
        return rad * np.cos(ang), rad * np.sin(ang)
    w = cr.draws(seed, call, B, H_out * W_out, 4)
    z = list(pair(w[0], w[1])) + list(pair(w[2], w[3]))
    if C_stage > 4:
        w5 = cr.draws(seed, call, B, H_out * W_out, 5)
        z.append(pair(w5[0], w5[1])[0])
    z = np.stack(z[:C_stage], axis=1).astype(np.float32).reshape(B, C_stage, H_out, W_out)
    return np.float32(scale) * z


# ---- shared by the two test files ----------------------------------------------------------------------------------------------
# the image keys of configs/config_SVR.yaml, with two keys the transformation must ignore
SVR_CFG = dict(image_add_grayscale=True, image_means=[0.03492457, 0.03379815, 0.03475684, 0.03874264], image_noise=False,
               image_noise_scale=0.02, image_normalize=True, image_pad=False, image_pad_size=[0, 0], image_remove_alpha=True,
               image_resize=True, image_size=[224, 224], image_stds=[0.10963749, 0.10795733, 0.11031612, 0.12266339],
               images_fname='ShapeNetAll13_images.h5', batch_size=128)
RESIZE_BAR = 2.0**-14          # the stand-in forms the source coordinate in float32 (ulp near 137: 2^-16) on values in [0, 1]


def case(fx, name):
    """(source images, config, recorded noise or None, the reference's output) of one fixture configuration."""
    name = str(name)
    return (fx['images_' + str(fx['src_' + name])], json.loads(str(fx['cfg_' + name])),
            fx['noise_' + name] if 'noise_' + name in fx.files else None, fx['out_' + name])


def resize_bound(cfg, c_out):
    """|restatement - stand-in| allowed per output channel on a Resize configuration: 2^-14 / std_c (2^-14 unnormalised)."""
    if not cfg.get('image_normalize'):
        return np.full((1, c_out, 1, 1), RESIZE_BAR)
    return (RESIZE_BAR / np.asarray(cfg['image_stds'], np.float64)[:c_out]).reshape(1, c_out, 1, 1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
