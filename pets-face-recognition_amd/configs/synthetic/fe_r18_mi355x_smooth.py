# ResNet-18 FE + ArcFace on 1xMI355X with a label-smoothed cross-entropy instead of the focal loss:
# SoftmaxBasedMetricLearning(..., is_focal=False, loss_kwargs=dict(label_smoothing=0.1)) -> nn.CrossEntropyLoss(label_smoothing=0.1),
# run inside the fused head's row kernel (losses/__init__.py:_fusable)
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=12, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=40,
      is_focal=False, loss_kwargs=dict(label_smoothing=0.1))
