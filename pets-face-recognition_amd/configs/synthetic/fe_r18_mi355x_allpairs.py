# ResNet-18 FE + ArcFace on 1xMI355X with ALL-PAIRS verification: next to the sampled-pair metrics the evaluation bins the score of every pair
# of the validation set (match.pair_histogram: the match GEMM with a histogram epilogue, nothing N x N is written) and reports
# 'AllPairs ROC AUC', 'AllPairs EER' and, per entry of all_pairs_far, 'AllPairs TAR@FAR=...' / 'AllPairs TH@FAR=...' (engine/metrics.py
# HistStats).  A sampled list of ~10^4 impostor pairs resolves FAR 1e-3 at best; N embeddings give N (N - 1) / 2 pairs.
# all_pairs_bins (default 4096) is the histogram resolution over cos in [-1, 1]; match_dtype selects the GEMM operand as for Recall@K.
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=40, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=160)
all_pairs_far = [1e-1, 1e-2, 1e-3]
all_pairs_bins = 4096
