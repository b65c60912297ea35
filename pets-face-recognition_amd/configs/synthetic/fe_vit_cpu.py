# A tiny ViT (2 layers, 192 wide, 3 heads, patch 8 at 32x32) FE + ArcFace, bs=8, PyTorch CPU via main.py (plumbing)
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

MODEL_KWARGS = dict(image_size=32, patch_size=8, num_layers=2, num_heads=3, hidden_dim=192, mlp_dim=384)
_make(globals(), arch='vit_t_16', n_train_ids=12, n_val_ids=4, photos=4, image_size=32, train_bs=8, test_bs=8,
      device='cpu', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '2')), n_pairs=10,
      optimizer_kind='adamw', model_kwargs=MODEL_KWARGS)
