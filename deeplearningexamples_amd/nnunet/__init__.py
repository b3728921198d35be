"""nnU-Net (BraTS22 UNet3D) inference: reference PyTorch/Segmentation/nnUNet."""
