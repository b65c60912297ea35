# ResNet-18 FE trained CENTRE-FREE on 1xMI355X with the MULTI-SIMILARITY loss and its miner (Wang et al., CVPR 2019) against a
# cross-batch memory of 4096 past embeddings (losses/pair.py: PairLoss('multi_similarity', memory=4096), csrc/pfr_pairmine.hip).  An
# extremes pass finds the hardest positive and negative of every anchor over the batch and the ring; a second pass keeps the negatives
# with s + epsilon > s_p* and the positives with s - epsilon < s_n* and sums the two log(1 + sum exp) terms.  The mining is a constant in
# the gradient; the mean runs over the valid anchors (the published code divides by the batch size).  The first 16 calls fill the ring
# without using it.  The ring is rank-local and not checkpointed.
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=12, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=int(os.environ.get('PFR_N_EPOCHS', '1')), limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=40,
      pair_loss=dict(kind='multi_similarity', alpha=2.0, beta=50.0, base=0.5, epsilon=0.1, memory=4096,
                     memory_warmup=int(os.environ.get('PFR_XBM_WARMUP', '16'))), pk=(8, 4), centre_free=True)
