# ResNet-18 FE + MagFace (Meng et al., CVPR 2021) on 1xMI355X: the angular margin grows with the embedding's length and a regulariser
# on the length is part of the loss, so that |emb| becomes a per-photo quality score (SoftmaxBasedMetricLearning(..., margin='magface'):
# losses/large_margin.py MagFaceProduct, no buffers).  The head stays one fused path: one small launch prepares the per-row margins and
# the regulariser's values, the margin + cross-entropy row kernel also writes d loss / d |emb|, and the embedding backward adds the
# radial term in the pass that writes the tangent one.  The Trainer's loss line shows the regulariser as `loss_g`; `quality = True`
# makes the validation report the embeddings' mean length ('Quality mean norm') and how well it orders the genuine pairs' scores.
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=12, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=int(os.environ.get('PFR_N_EPOCHS', '1')), limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=40,
      margin='magface', margin_kwargs=dict(l_a=10, u_a=110, l_m=0.45, u_m=0.8, lambda_g=35.0))
quality = True
