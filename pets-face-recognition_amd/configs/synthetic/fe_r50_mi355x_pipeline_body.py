# The fe_r50_mi355x_pipeline workload on the data layout and order of the reference's body configs (body_dog_fe.py:18-33), 256 x 256
# network input: ragged raw frames → resize_with_padding (thumbnail + centred zero pad, csrc/pfr_augment_fit.hip) → RandomCrop(252) →
# Resize(256) → RandomRotation(5) → sharpness / autocontrast on the rotated image → ToTensor, all on the device.
# THROUGHPUT RUN ONLY: with ragged=True and noise_bank=64 the dataset hands out 64 pre-rendered frames (frame i % 64 whatever the label,
# data_loading/synthetic.py), the per-item cost of a cached, already decoded crop.  The images carry no learnable signal.
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet50', n_train_ids=10000, n_val_ids=int(os.environ.get('PFR_VAL_IDS', '200')), photos=4, image_size=256, train_bs=256, test_bs=64,
      device='cuda:0', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '60')),
      workers=int(os.environ.get('PFR_WORKERS', '16')), device_augment=True, noise_bank=64,
      ragged=True, pipeline='body')
