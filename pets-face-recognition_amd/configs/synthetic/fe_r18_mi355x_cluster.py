# ResNet-18 FE + ArcFace on 1xMI355X with IDENTITY CLUSTERING of the validation set next to the verification metrics: which items are
# the same animal, and how many distinct animals are there?  Single linkage at a similarity threshold = the connected components of the
# pairs at or above it, united in the epilogue of the match GEMM (csrc/pfr_cluster.hip: a lock-free union-find on a parent array, no
# N x N score matrix, no edge list), scored against the classes: 'Cluster F / precision / recall thr=…' (pairwise), 'Cluster BCubed F
# thr=…' and 'Clusters thr=…'.  Thresholds are similarities (cos + 1) / 2 like 'Opt thr'; 'opt' is the run's own optimal threshold.
# Not covered: other linkages (average, DBSCAN, Chinese whispers); a threshold so low that the graph is near complete is correct but slow.
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=40, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=160)
cluster = dict(thresholds=[0.8, 'opt'])
