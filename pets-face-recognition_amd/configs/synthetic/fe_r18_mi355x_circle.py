# ResNet-18 FE + ArcFace + Circle loss (Sun et al., CVPR 2020) on 1xMI355X: the identity loss of the margin head plus a pair loss on the
# batch's own Gram matrix, loss = head + 0.5 * circle (SoftmaxBasedMetricLearning(..., pair_loss=dict(kind='circle', weight=0.5)):
# losses/pair.py).  The pair term is one forward and one backward launch around the embedding's L2 normalisation
# (csrc/pfr_pairloss.hip); nothing B x B is written.  Batches are P x K = 8 identities x 4 photos (data_loading.PKBatchSampler), so every
# anchor has 3 positives and 28 negatives.  The Trainer's loss line shows the pair term as `loss_pair`.  Rank-local: no all-gather.
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=12, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=int(os.environ.get('PFR_N_EPOCHS', '1')), limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=40,
      pair_loss=dict(kind='circle', weight=0.5, m=0.25, gamma=64.0), pk=(8, 4))
