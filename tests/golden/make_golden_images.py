#!/usr/bin/env python3
"""Generate g23_images.npz by running the GENUINE reference's image transformations on CPU.

Build-container only, like make_golden_clouds.py: the reference is imported, never copied; only data is written.  The reference
module is loaded by file path; torchvision is absent, so torchvision.transforms.Compose gets the stand-in make_golden_clouds.py uses.

cv2 is absent too.  Its only use in the module is cv2.resize(img_hwc, (w, h)) on float32 (bilinear, the default).  The stand-in
below answers that one call with torch.nn.functional.interpolate(mode='bilinear', align_corners=False) on CPU: an INDEPENDENT
implementation of the same half-pixel rule (source coordinate (d + 0.5) * n_src / n_dst - 0.5, clamped at the borders, no
antialiasing).  It is not cv2: it forms the coordinate in float32, cv2 in float64, so on the Resize configurations the fixture pins
the rule to about 2^-14 of the value range, not the bits.  Parity with the real cv2 has not been run.

The noise the reference draws (np.random.normal under the global seed) is recorded as np.float32(RandomState(seed).normal(...)),
the value it adds, so that a test can feed it explicitly.

    python tests/golden/make_golden_images.py
"""
import importlib.util
import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
if not os.path.isdir(REF):
    sys.exit('reference checkout not present: fixtures can only be regenerated in the build container')

import numpy as np
import torch


class _Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, sample):
        for t in self.transforms:
            sample = t(sample)
        return sample


def _resize(img_hwc, size):
    w, h = size
    x = torch.from_numpy(np.ascontiguousarray(img_hwc, dtype=np.float32)).permute(2, 0, 1)[None]
    y = torch.nn.functional.interpolate(x, size=(h, w), mode='bilinear', align_corners=False)
    return y[0].permute(1, 2, 0).contiguous().numpy()


sys.modules['torchvision'] = types.ModuleType('torchvision')
sys.modules['torchvision.transforms'] = types.ModuleType('torchvision.transforms')
sys.modules['torchvision.transforms'].Compose = _Compose
sys.modules['cv2'] = types.ModuleType('cv2')
sys.modules['cv2'].resize = _resize

spec = importlib.util.spec_from_file_location('ref_image_transformations', os.path.join(REF, 'lib', 'datasets', 'image_transformations.py'))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

# the values of configs/config_SVR.yaml (settings, not program text)
SVR_MEANS = [0.03492457, 0.03379815, 0.03475684, 0.03874264]
SVR_STDS = [0.10963749, 0.10795733, 0.11031612, 0.12266339]
MEANS5, STDS5 = [0.05, 0.04, 0.03, 0.02, 0.5], [0.2, 0.11, 0.12, 0.13, 0.4]
NOISE_SEED = 2301

# name -> (source set, config).  Source 'a': 3 images (3, 9, 7); source 'b': 2 images (4, 6, 6).
CONFIGS = {
    'tonumpy': ('a', {}),
    'tonumpy4': ('b', {}),
    'pad': ('a', dict(image_pad=True, image_pad_size=[2, 1])),
    'gray': ('a', dict(image_add_grayscale=True)),
    'gray_norm': ('a', dict(image_add_grayscale=True, image_normalize=True, image_means=SVR_MEANS, image_stds=SVR_STDS)),
    'gray_norm_alpha': ('b', dict(image_add_grayscale=True, image_normalize=True, image_means=MEANS5, image_stds=STDS5,
                                  image_remove_alpha=True)),
    'resize_up': ('a', dict(image_resize=True, image_size=[12, 10])),
    'resize_down': ('a', dict(image_resize=True, image_size=[4, 3])),
    # the flag set of config_SVR.yaml (resize, grayscale, normalise, remove alpha; pad and noise off) at a small target size
    'svr': ('a', dict(image_resize=True, image_size=[16, 16], image_pad=False, image_pad_size=[0, 0], image_add_grayscale=True,
                      image_normalize=True, image_means=SVR_MEANS, image_stds=SVR_STDS, image_noise=False, image_noise_scale=0.02,
                      image_remove_alpha=True)),
    'noise': ('a', dict(image_noise=True, image_noise_scale=0.3)),
    'noise5': ('b', dict(image_add_grayscale=True, image_noise=True, image_noise_scale=0.3, image_remove_alpha=True)),
}


def main():
    rng = np.random.RandomState(23)
    src = {'a': rng.randint(0, 256, (3, 3, 9, 7)).astype(np.uint8), 'b': rng.randint(0, 256, (2, 4, 6, 6)).astype(np.uint8)}
    src['a'][0, :, 0, :3] = [[0, 255, 1]] * 3                   # the ends of the byte range, wherever the draw left them out
    data = {'images_a': src['a'], 'images_b': src['b'], 'names': np.array(list(CONFIGS))}
    for name, (s, cfg) in CONFIGS.items():
        compose = ref.ComposeImageTransformation(**cfg)
        outs, noises = [], []
        for i, image in enumerate(src[s]):
            np.random.seed(NOISE_SEED + i)
            out = compose(image)
            assert out.dtype == np.float32, (name, out.dtype)
            outs.append(out)
            if cfg.get('image_noise'):
                c_stage = image.shape[0] + (1 if cfg.get('image_add_grayscale') else 0)
                noises.append(np.float32(np.random.RandomState(NOISE_SEED + i).normal(
                    scale=cfg['image_noise_scale'], size=(c_stage,) + out.shape[1:])))
        data['out_' + name] = np.stack(outs)
        data['src_' + name] = np.array(s)
        data['cfg_' + name] = np.array(json.dumps(cfg))
        if noises:
            data['noise_' + name] = np.stack(noises)
    path = os.path.join(HERE, 'g23_images.npz')
    np.savez_compressed(path, **data)
    print(f'wrote {path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
