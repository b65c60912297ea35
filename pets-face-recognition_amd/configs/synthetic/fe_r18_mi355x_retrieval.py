# ResNet-18 FE + ArcFace on 1xMI355X with the RETRIEVAL METRICS of the re-ID literature next to Recall@K: 'mAP', 'mINP', 'CMC@K=...' and
# 'Mean first rank', from the exact rank of every positive of every query among all the other items of the validation set.  The ranks are
# counted in the epilogue of the match GEMM (csrc/pfr_rankcount.hip): no N x N score matrix, no argsort.  ks = the CMC ranks reported.
# Not covered: camera / junk filtering of the re-ID protocols, and the mAP of a re-ranked order.
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=40, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=160)
retrieval = dict(ks=[1, 5, 10])
