# IResNet-18 (models/iresnet.py) FE + ArcFace at 32x32 (input_size=32: fc sees a 2x2 map), bs=8, PyTorch CPU via main.py (plumbing)
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

MODEL_KWARGS = dict(input_size=32)
_make(globals(), arch='iresnet18', n_train_ids=12, n_val_ids=4, photos=4, image_size=32, train_bs=8, test_bs=8,
      device='cpu', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '2')), n_pairs=10,
      model_kwargs=MODEL_KWARGS)
