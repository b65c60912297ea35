# ResNet-18 FE + ArcFace on 1xMI355X with DBSCAN IDENTITY CLUSTERING of the validation set next to the verification metrics: an item is
# core when min_samples items (itself included) are at or above the similarity threshold; clusters are the components of the core items,
# a non-core item joins the cluster of its best core neighbour, everything else is noise.  Two passes of the match GEMM
# (csrc/pfr_dbscan.hip: a degree epilogue, then a union-find / border-key epilogue; no N x N score matrix, no edge list), scored against
# the classes with every noise item as a cluster of its own: 'DBSCAN F / precision / recall thr=…' (pairwise), 'DBSCAN BCubed F thr=…',
# 'DBSCAN clusters thr=…' and 'DBSCAN noise thr=…'.  Thresholds are similarities (cos + 1) / 2 like 'Opt thr'; 'opt' is the run's own
# optimal threshold.  min_samples=3 with 4 photos per animal: an animal's photos are core when they all see two of the others.
# Not covered: average linkage, HDBSCAN / OPTICS; a threshold so low that the graph is near complete is correct but slow.
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=40, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=160)
dbscan = dict(thresholds=[0.8, 'opt'], min_samples=3)
