# ResNet-18 FE + ArcFace on 1xMI355X with K-RECIPROCAL RE-RANKING of the match lists: next to 'Recall@K=...' of the cosine order the
# evaluation reports 'Rerank Recall@K=...' of the order match.rerank gives (Zhong et al., CVPR 2017: k-reciprocal neighbour sets and their
# expansion, Gaussian weights, local query expansion over k2 neighbours, Jaccard distance blended with the cosine distance by lambda_value).
# The sparse kernels (csrc/pfr_rerank.hip) keep rows of E = (k1 + 1) + (k1 + 1)(round(k1 / 2) + 1) and k2 * E entries per item: nothing
# N x N is built.  Optional key: candidates (default max(K, 100)) — only that many best cosine matches per query are re-ranked.
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=40, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=160)
rerank = dict(k1=20, k2=6, lambda_value=0.3)
