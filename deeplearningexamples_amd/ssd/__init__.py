"""SSD300 (Detection/SSD) on the gfx950 library: COCO detection inference with the decode, NMS and selection on the device."""
