# ResNet-18 FE + ArcFace with Partial FC (An et al., CVPR 2022) on 1xMI355X: every step scores the batch's own identities plus random
# negatives, a tenth of the class centres in all (SoftmaxBasedMetricLearning(..., sample_rate=0.1)), and with sparse_grad=True the head
# weight's gradient stays row-sparse (weight.row_grad): FusedSGD updates only the sampled rows and their momentum.  A torch optimizer
# would silently skip the head weight (its .grad is None): keep sparse_grad=False with anything but FusedSGD.
# 400 identities so that int(0.1 * 400) = 40 sampled classes hold a batch of 32.
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=400, n_val_ids=12, photos=2, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=20,
      sample_rate=0.1, sparse_grad=True)
