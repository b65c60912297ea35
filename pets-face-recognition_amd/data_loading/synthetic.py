"""Synthetic stand-in for the reference's folder-per-identity `RecDataset` (/root/reference/data_loading/dataset.py:
67-201): same item contract `{'x': float 3xHxW in [0,1], 'label': int64, 'index': int64}` (dataset.py:125), same
`get_users()/get_labels()` surface used by the configs, but images are generated (datasets need network downloads).
Each identity has a fixed random low-frequency pattern; photos are the pattern plus noise, so that embeddings can
actually separate identities."""
import numpy as np
import torch
from torch.utils.data import Dataset


class SyntheticRecDataset(Dataset):
    def __init__(self, n_identities, photos_per_identity, image_size=224, seed=0, noise=0.15, raw_uint8=False, noise_bank=0, ragged=False, landmarks=False,
                 masks=False):
        self.n_id, self.ppi, self.size, self.seed, self.noise = n_identities, photos_per_identity, image_size, seed, noise
        # noise_bank = K > 0: the per-photo noise comes from K pre-drawn frames (photo i uses frame i % K) instead of a fresh
        # 150 k-sample draw per item — a loader whose per-item cost is that of a cached, already decoded frame (throughput runs)
        self.noise_bank = None
        if noise_bank:
            g = torch.Generator().manual_seed(seed * 104729 + 17)
            self.noise_bank = noise * torch.randn(int(noise_bank), 3, image_size, image_size, generator=g)
        # raw_uint8: hand out the HWC uint8 frame the reference's dataset holds BEFORE its transform (dataset.py:100-121);
        # the augmentation then runs on the device for the whole batch (data_loading/augment.py)
        self.raw_uint8 = raw_uint8
        # ragged: every item has its own seeded size (sides 64..1400, aspect 1:3..3:1), like the detector's raw crops the reference's
        # simple / no-align / body configs read; needs raw_uint8 and data_loading.ragged.ragged_collate
        if ragged and not raw_uint8:
            raise ValueError("SyntheticRecDataset: ragged=True hands out uint8 HWC frames (raw_uint8=True)")
        self.ragged = ragged
        # ragged + noise_bank = K: K whole FRAMES are rendered once, here (slot k: the size and noise of item k, the pattern of identity
        # k % n_identities) and item i hands out frame i % K — the per-item cost of a cached, already decoded crop.  The content then does
        # not follow the label: throughput runs only, like noise_bank itself
        self.frame_bank = None
        if ragged and noise_bank:
            bank, self.noise_bank = self.noise_bank, None
            self.frame_bank = [self._render(k % n_identities, self.item_size(k), bank[k]) for k in range(bank.shape[0])]
        # landmarks: every ragged item also carries 'pts', float64 [3, 2] = (x, y): three seeded landmarks (the triangle of `base_pts` under
        # a per-item rotation, scale and shift, well inside the frame and pairwise more than 5 px apart) - what the reference's landmark
        # models hand to preprocessor/align.py; masks: also 'mask', uint8 [H, W], a seeded ellipse (the detector's mask of PreprocCombined).
        # Both feed data_loading.align.DeviceAlign; the frames themselves are what they are without the two options
        if (landmarks or masks) and not ragged:
            raise ValueError("SyntheticRecDataset: landmarks / masks go with the ragged raw frames (ragged=True)")
        self.landmarks, self.masks = landmarks, masks
        self.labels = torch.arange(n_identities).repeat_interleave(photos_per_identity)
        self.label_map = {u: u for u in range(n_identities)}
        # identity -> dataset indices, the attribute the reference's PairGenerator samples from (dataset.py:93-96)
        self.uid_to_indices = {u: list(range(u * photos_per_identity, (u + 1) * photos_per_identity)) for u in range(n_identities)}

    def __len__(self):
        return self.n_id * self.ppi

    def get_users(self):
        return list(range(self.n_id))

    def get_labels(self):
        return self.labels.tolist()

    def _pattern(self, ident, hw=None):
        g = torch.Generator().manual_seed(self.seed * 1000003 + ident)
        low = torch.rand(3, 7, 7, generator=g)
        return torch.nn.functional.interpolate(low[None], size=hw or (self.size, self.size), mode='bilinear', align_corners=False)[0]

    def item_size(self, i):
        """(H, W) of item i"""
        if not self.ragged:
            return self.size, self.size
        from .ragged import seeded_size
        return seeded_size(self.seed * 15485863 + i)

    _BASE = ((0.3125, 0.36), (0.6875, 0.36), (0.5, 0.72))      # the landmark triangle in a unit crop: two eyes and the nose

    @classmethod
    def base_pts(cls, dsize):
        """the landmarks' place in an aligned (h, w) crop: float64 [3, 2] = (x, y)"""
        return np.asarray(cls._BASE, np.float64) * np.array([dsize[1], dsize[0]], np.float64)

    def item_landmarks(self, i):
        """float64 [3, 2] = (x, y) in item i's frame; every coordinate within 10 % .. 90 % of its side, sides of at least 64 px"""
        H, W = self.item_size(i)
        rs = np.random.RandomState((self.seed * 32452843 + i) % (2 ** 31))
        th, k = np.deg2rad(rs.uniform(-20, 20)), rs.uniform(0.9, 1.2) * min(H, W)
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        centre = np.array([W, H]) * (0.5 + rs.uniform(-0.02, 0.02, 2))
        return (np.asarray(self._BASE) - 0.5) @ R.T * k + centre + rs.uniform(-0.01, 0.01, (3, 2)) * min(H, W)

    def item_mask(self, i):
        """uint8 [H, W]: 1 inside a seeded ellipse around the frame's centre"""
        H, W = self.item_size(i)
        rs = np.random.RandomState((self.seed * 49979687 + i) % (2 ** 31))
        ry, rx = rs.uniform(0.40, 0.48, 2)
        yy, xx = np.mgrid[0:H, 0:W]
        return (((yy - H / 2) / (ry * H)) ** 2 + ((xx - W / 2) / (rx * W)) ** 2 <= 1.0).astype(np.uint8)

    def _extras(self, i):
        e = {}
        if self.landmarks:
            e['pts'] = torch.from_numpy(self.item_landmarks(i))
        if self.masks:
            e['mask'] = torch.from_numpy(self.item_mask(i))
        return e

    def _render(self, ident, hw, nz):
        nz = torch.nn.functional.interpolate(nz[None], size=hw, mode='nearest')[0]
        x = (self._pattern(ident, hw) + nz).clamp_(0, 1)
        return (x * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()

    def __getitem__(self, i):
        ident = int(self.labels[i])
        if self.frame_bank is not None:
            return {'x': self.frame_bank[i % len(self.frame_bank)], 'label': torch.tensor(self.label_map[ident], dtype=torch.int64),
                    'index': torch.tensor(i, dtype=torch.int64), **self._extras(i)}
        hw = self.item_size(i) if self.ragged else None
        if self.noise_bank is not None:
            x = (self._pattern(ident) + self.noise_bank[i % self.noise_bank.shape[0]]).clamp_(0, 1)
        else:
            g = torch.Generator().manual_seed(self.seed * 7919 + i)
            h, w = hw or (self.size, self.size)
            x = (self._pattern(ident, hw) + self.noise * torch.randn(3, h, w, generator=g)).clamp_(0, 1)
        if self.raw_uint8:
            x = (x * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
        return {'x': x, 'label': torch.tensor(self.label_map[ident], dtype=torch.int64), 'index': torch.tensor(i, dtype=torch.int64),
                **self._extras(i)}


class RecSubset(Dataset):
    def __init__(self, dataset, indices):
        self.dataset, self.indices = dataset, list(indices)

    def __len__(self):
        return len(self.indices)

    def __getitem__(self, i):
        return self.dataset[self.indices[i]]
