# A short MobileNetV2 (four inverted-residual rows, torchvision's widths) FE + ArcFace at 64x64, bs=8, PyTorch CPU via main.py (plumbing)
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

MODEL_KWARGS = dict(inverted_residual_setting=[[1, 16, 1, 1], [6, 24, 2, 2], [6, 32, 2, 2], [6, 64, 1, 1]])
_make(globals(), arch='mobilenet_v2', n_train_ids=12, n_val_ids=4, photos=4, image_size=64, train_bs=8, test_bs=8,
      device='cpu', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '2')), n_pairs=10,
      model_kwargs=MODEL_KWARGS)
