"""Data pipeline: torchvision-free ImageFolder + transforms, synthetic ImageNet-shaped sources,
and ``create_dataloaders`` with the reference signature (GM/data_setup.py:12-65)."""
from .batch_mix import BatchMix, MixPlan, mix_reference
from .color_augment import ColorAugment, ColorPlan, color_reference
from .device_input import DeviceInput, RandomResizedCropFlip, center_box, full_box
from .image_folder import IMG_EXTENSIONS, ImageFolder, pil_loader
from .loaders import NUM_WORKERS, create_dataloaders, create_synthetic_dataloaders
from .prefetch import DevicePrefetcher, prefetch
from .random_erasing import ErasePlan, RandomErasing, erase_reference
from .synthetic import DeviceSyntheticLoader, SyntheticImageNet
from . import transforms

__all__ = ["ImageFolder", "pil_loader", "IMG_EXTENSIONS", "create_dataloaders", "create_synthetic_dataloaders",
           "NUM_WORKERS", "SyntheticImageNet", "DeviceSyntheticLoader", "DevicePrefetcher", "prefetch", "transforms",
           "DeviceInput", "RandomResizedCropFlip", "full_box", "center_box", "BatchMix", "MixPlan", "mix_reference",
           "ErasePlan", "RandomErasing", "erase_reference", "ColorAugment", "ColorPlan", "color_reference"]
