"""The preprocessed data directory of the reference (data_preprocessing/preprocessor.py writes it; data_loading/data_module.py and
dali_loader.py read it) with numpy and pickle alone: <case>_x.npy [C, D, H, W] images, <case>_y.npy [1, D, H, W] labels,
<case>_meta.npy [4, 3] = (crop minimum, crop maximum, original shape, cropped shape), config.pkl.  No DALI, no Lightning."""
import glob
import os
import pickle

import numpy as np


def data_paths(data, task, dim, exec_mode, benchmark):
    """(directory of the .npy files, directory of config.pkl) as the reference derives them (data_module.py:108-114, utils/utils.py:
    30-40): a --data other than the default /data is both; the default means /data/<task>_<dim>d, and a prediction run that is no
    benchmark reads the files of its test/ subdirectory."""
    if data != "/data":
        return data, data
    base = os.path.join(data, "%s_%dd" % (task, dim))
    return (os.path.join(base, "test") if exec_mode == "predict" and not benchmark else base), base


def load_config(data_dir):
    """config.pkl (utils/utils.py:34-40): patch_size, spacings, n_class, in_channels."""
    path = os.path.join(data_dir, "config.pkl")
    if not os.path.exists(path):
        raise FileNotFoundError("nnU-Net: %s not found (run the reference's preprocess.py for task 11 / 12)" % path)
    with open(path, "rb") as f:
        return pickle.load(f)


def load_data(path, pattern, non_empty=True):
    data = sorted(glob.glob(os.path.join(path, pattern)))
    if non_empty and not data:
        raise FileNotFoundError("No data found in %s with pattern %s" % (path, pattern))
    return data


def kfold_split(n, nfolds, fold, seed=12345):
    """(train_idx, val_idx) of sklearn's KFold(n_splits=nfolds, shuffle=True, random_state=12345).split(range(n)) for one fold
    (data_module.py:93-94), restated: indices shuffled by numpy's RandomState(seed), consecutive folds of n // nfolds elements, the
    first n % nfolds one longer; both index lists ascending."""
    if not 2 <= nfolds <= n:
        raise ValueError("Cannot have number of splits n_splits=%d greater than the number of samples: n_samples=%d." % (nfolds, n))
    idx = np.arange(n)
    np.random.RandomState(seed).shuffle(idx)
    sizes = np.full(nfolds, n // nfolds, dtype=int)
    sizes[:n % nfolds] += 1
    start = int(sizes[:fold].sum())
    mask = np.zeros(n, dtype=bool)
    mask[idx[start:start + sizes[fold]]] = True
    return np.nonzero(~mask)[0], np.nonzero(mask)[0]


def test_files(data_dir, exec_mode, nfolds, fold):
    """(images, metas) of get_test_fnames (data_module.py:97-105)."""
    imgs, meta = load_data(data_dir, "*_x.npy", non_empty=False), load_data(data_dir, "*_meta.npy", non_empty=False)
    if exec_mode == "predict" and "val" in data_dir:
        _, val = kfold_split(len(imgs), nfolds, fold)
        imgs = sorted(np.array(imgs)[val].tolist())
        meta = sorted(np.array(meta)[val].tolist()) if meta else meta
    return imgs, meta


def fold_files(data_dir, nfolds, fold):
    """((train images, train labels), (val images, val labels)) of DataModule.setup (data_module.py:52-60)."""
    imgs, lbls = load_data(data_dir, "*_x.npy"), load_data(data_dir, "*_y.npy")
    tr, va = kfold_split(len(imgs), nfolds, fold)
    pick = lambda files, idx: list(np.array(files)[idx])
    return (pick(imgs, tr), pick(lbls, tr)), (pick(imgs, va), pick(lbls, va))


def center_crop_pad(img, patch):
    """dali_loader.py:76-77 for the benchmark pipeline: fn.crop(crop=patch, out_of_bounds_policy="pad") -- a centred window of the
    patch size, zeros outside the image.  DALI anchors the window at round-half-down of (size - patch) / 2."""
    out = np.zeros(img.shape[:1] + tuple(patch), dtype=img.dtype)
    src, dst = [slice(None)], [slice(None)]
    for size, p in zip(img.shape[1:], patch):
        a = (size - p) // 2 if size >= p else -((p - size) // 2)
        s0, s1 = max(a, 0), min(a + p, size)
        src.append(slice(s0, s1))
        dst.append(slice(s0 - a, s1 - a))
    out[tuple(dst)] = img[tuple(src)]
    return out
