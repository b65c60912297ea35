# ResNet-18 FE + AdaFace (Kim et al., CVPR 2022) on 1xMI355X: the margin of every sample follows its feature norm, a proxy of image
# quality, so that blurred, tiny or occluded crops do not dominate the gradient (SoftmaxBasedMetricLearning(..., margin='adaface'):
# losses/large_margin.py AdaFaceProduct, persistent buffers batch_mean / batch_std).  The whole head stays one fused path: one small
# launch prepares the per-row margins, the margin + cross-entropy row kernel reads them.
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=12, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=40,
      margin='adaface', margin_kwargs=dict(m=0.4, h=0.333))
