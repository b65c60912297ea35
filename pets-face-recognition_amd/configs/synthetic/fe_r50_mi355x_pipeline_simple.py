# The fe_r50_mi355x_pipeline workload on the data layout of the reference's simple / no-align configs (simple_fe_dog.py:17-31): the
# loader hands out the detector's raw crops, every frame with its own size, as a ragged batch (data_loading/ragged.py); on the device
# sharpness / autocontrast act on the raw frame, Resize((224, 224)) brings the batch to one canvas (csrc/pfr_augment_fit.hip), then
# RandomCrop(220) → Resize(224) → RandomRotation(5) → ToTensor as in the head pipeline.
# THROUGHPUT RUN ONLY: with ragged=True and noise_bank=64 the dataset hands out 64 pre-rendered frames (frame i % 64 whatever the label,
# data_loading/synthetic.py), the per-item cost of a cached, already decoded crop.  The images carry no learnable signal.
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet50', n_train_ids=10000, n_val_ids=int(os.environ.get('PFR_VAL_IDS', '200')), photos=4, image_size=224, train_bs=256, test_bs=64,
      device='cuda:0', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '60')),
      workers=int(os.environ.get('PFR_WORKERS', '16')), device_augment=True, noise_bank=64,
      ragged=True, pipeline='simple')
