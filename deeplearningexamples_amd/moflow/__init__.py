"""MoFlow molecule generation (reference: PyTorch/DrugDiscovery/MoFlow): the reverse flow on the kernels of csrc/moflow.hip."""
