# ResNet-18 FE trained CENTRE-FREE on 1xMI355X: no class head, the criterion is the supervised contrastive loss (Khosla et al., NeurIPS
# 2020, L_out, tau = 0.1) on the batch's own Gram matrix (losses.PairMetricLearning + losses/pair.py): the mode for identities that are too
# many, too few-shot or open-ended for a centre each.  Batches are P x K = 8 identities x 4 photos (data_loading.PKBatchSampler); an anchor
# without a positive in its batch would contribute nothing.  `loss` and the Trainer's `loss_pair` column are the same number here
# (weight 1).  Rank-local: no all-gather.
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=12, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=int(os.environ.get('PFR_N_EPOCHS', '1')), limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=40,
      pair_loss=dict(kind='supcon', tau=0.1), pk=(8, 4), centre_free=True)
