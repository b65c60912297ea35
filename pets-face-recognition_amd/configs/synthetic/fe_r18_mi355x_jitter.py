# ResNet-18 FE + ArcFace on 1xMI355X with the head pipeline on the device (fe_dogs_config.py:17-32) plus the colour / flip / erasing
# transforms of the reference's keypoint and mask configs (ColorJitter -> RandomAdjustSharpness -> RandomAutocontrast -> ToTensor ->
# RandomErasing) and the mirror flip that is the default augmentation of face recognition: RandomHorizontalFlip(0.5),
# ColorJitter(0.2, 0.2, 0.2, 0.02), RandomErasing(p=0.25) - data_loading/augment.py, csrc/pfr_augment_color.hip
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import make as _make

_make(globals(), arch='resnet18', n_train_ids=100, n_val_ids=12, photos=4, image_size=224, train_bs=32, test_bs=20,
      device='cuda:0', n_epochs=1, limit_train_batches=int(os.environ.get('PFR_LIMIT_TRAIN_BATCHES', '8')), n_pairs=40,
      device_augment=True, augment_extra=dict(p_hflip=0.5, color_jitter=(0.2, 0.2, 0.2, 0.02), erasing=dict(p=0.25)))
run_name = 'resnet18 synthetic with jitter'
