# ResNet-18 FE trained CENTRE-FREE on 1xMI355X with a CROSS-BATCH MEMORY (Wang et al., CVPR 2020): the supervised contrastive loss of
# fe_r18_mi355x_supcon.py, but every anchor also pairs with a ring of the normalised embeddings of the last 4096 items
# (losses/pair.py: PairLoss(memory=...), csrc/pfr_pairmem.hip), which carry no gradient.  With P x K = 8 x 4 batches an anchor has 3
# positives and 28 negatives in its batch; the ring adds up to 4096 partners.  The first 16 calls fill the ring without using it (early
# features drift).  The ring is rank-local and not checkpointed: a resumed run starts with an empty one.
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=12, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=int(os.environ.get('PFR_N_EPOCHS', '1')), limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=40,
      pair_loss=dict(kind='supcon', tau=0.1, memory=4096, memory_warmup=int(os.environ.get('PFR_XBM_WARMUP', '16'))), pk=(8, 4), centre_free=True)
