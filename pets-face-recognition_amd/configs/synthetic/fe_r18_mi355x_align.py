# ResNet-18 FE + ArcFace on 1xMI355X on ALIGNED head crops, aligned on the device: ragged raw frames + three landmarks ->
# DeviceAlign(base_pts, (224, 224, 3)) (the reference's preprocessor/align.py: homography onto base_pts, warp to dsize -
# data_loading/align.py, csrc/pfr_align.hip) -> the head pipeline (fe_dogs_config.py:17-32) -> the network.  Training jitters the
# landmarks by 1 px (seeded), which a dataset aligned offline cannot offer; validation aligns on the landmarks as given.
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=12, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=40,
      device_augment=True, ragged=True, align=dict(jitter=1.0))
run_name = 'resnet18 synthetic, aligned on the device'
