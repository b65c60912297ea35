# ResNet-18 FE + ArcFace on 1xMI355X with the reference's commented-out trainer_kwargs switched on (fe_dogs_config.py:146-147):
# gradient_clip_val=1, gradient_clip_algorithm='norm' -> the fused optimizer's device-side clip_grad_norm_ before every step
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=12, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=40,
      gradient_clip_val=1.0, gradient_clip_algorithm='norm')
