"""Model registry — mirrors /root/reference/models/__init__.py (swin_t/s/b/l, SwinTransformer) and adds the
torchvision-compatible ResNets the reference's FE configs build (configs/dog_fe/fe_dogs_config.py:102-103) and the
torchvision-compatible ConvNeXt-T/S, MobileNetV2 and EfficientNet-B0..B3 of their alternative backbone lines
(configs/dog_fe/masked_head_dog.py:105-106, configs/dog_fe/fe_dogs_config.py:104-106), and the plain Vision Transformer with
torchvision's state-dict layout (vit_b_16 / vit_b_32 / vit_l_16, and the DeiT geometries vit_s_16 / vit_t_16 that keep head_dim 64):
`model_ = models.vit_b_16(); model_.heads = torch.nn.Linear(768, 512)`.  IResNet-18/34/50/100/200 carry the state-dict layout of the public
insightface arcface_torch backbone, the 112x112 face network the margin heads of losses/ were published with."""
from .resnet import ResNet, BasicBlock, Bottleneck, resnet18, resnet34, resnet50, resnet101  # noqa: F401
from .swin import SwinTransformer, swin_t, swin_s, swin_b, swin_l  # noqa: F401
from .convnext import ConvNeXt, convnext_tiny, convnext_small  # noqa: F401
from .mobilenet import MobileNetV2, InvertedResidual, mobilenet_v2  # noqa: F401
from .efficientnet import EfficientNet, MBConv, SqueezeExcitation, efficientnet_b0, efficientnet_b1, efficientnet_b2, efficientnet_b3  # noqa: F401
from .vit import VisionTransformer, EncoderBlock, vit_b_16, vit_b_32, vit_l_16, vit_s_16, vit_t_16  # noqa: F401
from .iresnet import IResNet, IBasicBlock, iresnet18, iresnet34, iresnet50, iresnet100, iresnet200  # noqa: F401
