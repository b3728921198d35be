"""HiFi-GAN (SpeechSynthesis/HiFiGAN) on the gfx950 library: mel-to-audio inference with the generator."""
