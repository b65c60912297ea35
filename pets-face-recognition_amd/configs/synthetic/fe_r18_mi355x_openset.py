# ResNet-18 FE + ArcFace on 1xMI355X with OPEN-SET IDENTIFICATION of the validation set next to the verification metrics: every item is
# searched against all the others (leave-one-out).  A probe with a mate is a hit when its best mate ranks before its best impostor; the
# threshold for a false-positive identification rate f is taken from the best impostor scores (each item searched against the gallery
# without its own class); 'OpenSet DIR@FPIR={f}' is the share of the mated probes that are hits at or above it (FNIR = 1 - DIR),
# 'OpenSet TH@FPIR={f}' the threshold as a similarity (cos + 1) / 2, 'OpenSet rank1' the hits without a threshold and 'OpenSet suspects'
# the number of items whose best impostor beats their best mate (label suspects).  One pass of the match GEMM (csrc/pfr_extremes.hip: a
# class-conditioned atomic-max epilogue; no N x N score matrix).  With 160 items floor(f n) is 16 and 1 for the two rates below.
# Not covered: more than one extreme per item (the top-K match lists do that).
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=40, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=160)
open_set = dict(fpir=[0.1, 0.01])
