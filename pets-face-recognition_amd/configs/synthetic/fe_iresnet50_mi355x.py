# IResNet-50 FE (models/iresnet.py: the insightface arcface_torch backbone, 112x112 crops, flatten → fc → features neck) + ArcFace,
# FusedSGD with backbone / `fc` + `features` / margin parameter groups (lr split), synthetic 10k ids, bs=256, MI355X bf16
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='iresnet50', n_train_ids=10000, n_val_ids=200, photos=4, image_size=112, train_bs=256, test_bs=64,
      device='cuda:0', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '20')), workers=8)
