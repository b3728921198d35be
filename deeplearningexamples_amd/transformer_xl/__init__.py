"""Transformer-XL language-model evaluation with memory (model.py, infer.py, eval.py)."""
