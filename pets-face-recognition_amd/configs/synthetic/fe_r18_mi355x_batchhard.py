# ResNet-18 FE + ArcFace + BATCH-HARD TRIPLET loss (Hermans et al. 2017, on cosine scores) on 1xMI355X: loss = head + 0.5 * batch_hard
# (SoftmaxBasedMetricLearning(..., pair_loss=dict(kind='batch_hard', weight=0.5)): losses/pair.py).  Per anchor the hardest positive (the
# lowest score of its identity) and the hardest negative (the highest score of another identity) of the batch are found by an extremes
# pass (csrc/pfr_pairmine.hip), l_i = max(0, s_n* - s_p* + m); the backward is sparse, two weights per anchor.  Batches are P x K = 8
# identities x 4 photos (data_loading.PKBatchSampler): 3 positives and 28 negatives per anchor.  The selection is a constant in the
# gradient, the mean runs over the valid anchors.  Rank-local: no all-gather.  gamma > 0 is the soft margin softplus(gamma z) / gamma.
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=12, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=int(os.environ.get('PFR_N_EPOCHS', '1')), limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=40,
      pair_loss=dict(kind='batch_hard', weight=0.5, m=0.3, gamma=0.0), pk=(8, 4))
