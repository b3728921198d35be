"""Temporal Fusion Transformer (PyTorch/Forecasting/TFT of the reference): host model, forecaster, data and command line."""
