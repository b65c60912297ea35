# ResNet-18 FE + CurricularFace (Huang et al., CVPR 2020) on 1xMI355X: ArcFace's margin on the target, and the negatives harder than
# the shifted target are re-weighted by t + cos, t the running mean of the target cosines: easy samples first, hard ones as training
# proceeds (SoftmaxBasedMetricLearning(..., margin='curricular'): losses/large_margin.py CurricularFaceProduct, persistent buffer t).
# The whole head stays one fused path: one small launch moves t, the margin + cross-entropy row kernel reads it.
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=12, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=40,
      margin='curricular', margin_kwargs=dict(m=0.5))
