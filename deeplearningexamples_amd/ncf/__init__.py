"""Neural Collaborative Filtering (NeuMF on ml-20m): inference and HR@K evaluation of the reference's
PyTorch/Recommendation/NCF recipe on the gfx950 library.  Training is not built."""
