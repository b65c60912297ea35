# ResNet-18 FE + ArcFace on 1xMI355X with the reference Trainer's `stochastic_weight_avg` switched on: from epoch
# int(0.5 * n_epochs) on a SWALR replaces the config's scheduler and the weights are averaged at the end of every epoch; after the
# last epoch the average becomes the model and its BatchNorm statistics are re-estimated over the train loader (utils.update_bn)
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=12, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=4, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=40,
      trainer_extra=dict(stochastic_weight_avg=True, swa_epoch_start=0.5, annealing_epochs=2))
