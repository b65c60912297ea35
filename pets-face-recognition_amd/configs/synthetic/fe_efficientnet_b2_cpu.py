# A short EfficientNet (four MBConv stages: a ratio-1 block with a residual, 5x5 at both strides, SE everywhere) FE + ArcFace at 64x64,
# bs=8, PyTorch CPU via main.py (plumbing)
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

MODEL_KWARGS = dict(inverted_residual_setting=[(1, 3, 1, 16, 16, 1), (6, 5, 2, 16, 24, 2), (6, 3, 2, 24, 40, 2), (6, 5, 1, 40, 48, 1)],
                    last_channel=192, dropout=0)
_make(globals(), arch='efficientnet_b2', n_train_ids=12, n_val_ids=4, photos=4, image_size=64, train_bs=8, test_bs=8,
      device='cpu', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '2')), n_pairs=10,
      model_kwargs=MODEL_KWARGS)
