from .synthetic import SyntheticRecDataset, RecSubset  # noqa: F401
from .pairs import PairGenerator  # noqa: F401
from .augment import DeviceAugmentation, train_augmentation, val_augmentation  # noqa: F401
from .augment import simple_train_augmentation, simple_val_augmentation, body_train_augmentation, body_val_augmentation  # noqa: F401
from .ragged import ragged_collate, pack_frames, unpack_frames, is_ragged  # noqa: F401
from .prefetch import DevicePrefetcher  # noqa: F401
from .align import DeviceAlign, align_torch, pack_masks, solve as align_solve  # noqa: F401
from .pk_sampler import PKBatchSampler  # noqa: F401
