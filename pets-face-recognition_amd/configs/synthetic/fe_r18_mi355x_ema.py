# ResNet-18 FE + ArcFace on 1xMI355X with an exponential moving average of the weights: Trainer(ema_decay=0.999) -> the EMA is
# updated inside the fused optimizer's step kernel; validation / test run on the averaged weights, the checkpoint's sidecar holds
# `averaged_state_dict` (eval_fe.py --averaged)
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=12, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=40,
      trainer_extra=dict(ema_decay=0.999))
