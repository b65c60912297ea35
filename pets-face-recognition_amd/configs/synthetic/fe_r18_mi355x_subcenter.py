# ResNet-18 FE + Sub-center ArcFace (Deng et al., ECCV 2020) on 1xMI355X: three centres per identity in the fused head
# (SoftmaxBasedMetricLearning(..., sub_centers=3): weight [3 * num_class, 512], class cosine = max of its three sub-cosines), with the
# label-smoothed cross-entropy of fe_r18_mi355x_smooth.py.  After training, `add_margin.prune_sub_centers()` keeps the dominant centre
# of every class and leaves a reference-shaped one-centre head.
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=12, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=40,
      is_focal=False, loss_kwargs=dict(label_smoothing=0.1), sub_centers=3)
