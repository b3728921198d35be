"""Which model family may import which.  Read from the source with `ast`; nothing of the package is imported.

A family is a directory of the package (bert, convnets, ..., waveglow).  Every family may import the shared layer -- utils,
functional, _cabi, multi_tensor, build -- and itself.  The shared layer imports no family.  An edge between two families must be
listed in ALLOWED, as a prefix of the imported module's dotted name, with its reason: what is shared belongs in `utils`, not in
whichever family needed it first."""
import ast
import os

PKG = "deeplearningexamples_amd"
ROOT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), PKG)
SHARED = {"utils", "functional", "_cabi", "multi_tensor", "build"}
ALLOWED = {
    "jasper": ("quartznet",),                                # the same network family: one configuration reader, front end, CTC tail
    "ssd": ("convnets",),                                    # the detector's trunk is the classifiers' ResNet-50 units
    "tacotron2": ("waveglow",),                              # one training script and one vocoder for both halves of the pipeline
    "fastpitch": ("hifigan", "waveglow", "tacotron2.text"),  # text front end and the two vocoders its command line drives
    "hifigan": ("waveglow",),                                # the denoiser and the wav writer
    "waveglow": ("tacotron2.audio", "tacotron2.data_function"),        # the mel front end of the training data
    "quartznet": ("tacotron2.audio",),                       # the mel filter bank and the wav reader
}


def _targets(node, here):
    """Dotted names, relative to the package, of what an import statement of module `here` (a list of path parts) brings in."""
    if isinstance(node, ast.Import):
        names = [a.name for a in node.names]
    elif node.level == 0:
        names = ["%s.%s" % (node.module, a.name) for a in node.names]
    else:
        base = here[:len(here) - node.level] + (node.module.split(".") if node.module else [])
        names = [".".join([PKG] + base + [a.name]) for a in node.names]
    return [n[len(PKG) + 1:] for n in names if n.startswith(PKG + ".")]


def _edges():
    for d, _, files in os.walk(ROOT):
        for f in files:
            if not f.endswith(".py"):
                continue
            path = os.path.join(d, f)
            here = os.path.relpath(path, ROOT)[:-3].split(os.sep)
            with open(path) as fh:
                tree = ast.parse(fh.read(), path)
            for node in ast.walk(tree):
                if isinstance(node, (ast.Import, ast.ImportFrom)):
                    for t in _targets(node, here):
                        yield here[0], t, "%s:%d" % (os.path.relpath(path, ROOT), node.lineno)


def test_cross_family_imports_are_listed():
    bad = []
    for src, target, where in _edges():
        dst = target.split(".")[0]
        if dst == src or dst in SHARED and src not in SHARED:
            continue
        if src in SHARED and dst in SHARED:
            continue
        if not any(target == a or target.startswith(a + ".") for a in ALLOWED.get(src, ())):
            bad.append("%s imports %s" % (where, target))
    assert not bad, "\n".join(sorted(bad))


def test_the_walk_sees_the_package():
    edges = list(_edges())
    assert ("jasper", "quartznet.infer.CTCRecognizer") in [(s, t) for s, t, _ in edges]
    assert any(s == "ssd" and t.startswith("convnets.infer.") for s, t, _ in edges)
    assert len({s for s, _, _ in edges}) >= 12
