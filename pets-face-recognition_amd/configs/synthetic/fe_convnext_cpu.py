# A short ConvNeXt (one block per stage, two in the third; ConvNeXt-T's widths) FE + ArcFace at 64x64, bs=8, PyTorch CPU via main.py (plumbing)
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

MODEL_KWARGS = dict(depths=(1, 1, 2, 1), dims=(96, 192, 384, 768))
_make(globals(), arch='convnext_tiny', n_train_ids=12, n_val_ids=4, photos=4, image_size=64, train_bs=8, test_bs=8,
      device='cpu', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '2')), n_pairs=10,
      optimizer_kind='adamw', model_kwargs=MODEL_KWARGS)
