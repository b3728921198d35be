"""Compile the reference's BERT LAMB optimizer modules to bytecode under oracle/_ref/ (never committed).

    make -C oracle            (run by __graft_entry__.build())

TEST INFRASTRUCTURE.  tests/test_gpu_lamb_reference.py::test_reference_class_steps_on_hip_kernels steps the reference's
unmodified FusedLAMBAMP class and PolyWarmUpScheduler on the GPU box, where the reference tree is not: the modules travel
there as sourceless .pyc files built here from the reference (lamb_amp_opt/fused_lamb/, schedulers.py).  Without the
reference tree this builds nothing and leaves what an earlier build made.
"""
import os
import py_compile
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle._ref_import import REF  # noqa: E402

BERT = os.path.join(REF, "PyTorch", "LanguageModeling", "BERT")
OUT = os.path.join(HERE, "_ref", "bert")
MODULES = ["schedulers.py", "lamb_amp_opt/fused_lamb/__init__.py", "lamb_amp_opt/fused_lamb/fused_lamb.py"]


def main():
    if not all(os.path.isfile(os.path.join(BERT, m)) for m in MODULES):
        print("oracle/_ref: no reference tree at %s, nothing built" % REF)
        return
    for m in MODULES:
        dst = os.path.join(OUT, m[:-len(".py")] + ".pyc")
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        py_compile.compile(os.path.join(BERT, m), cfile=dst, dfile=m, doraise=True)
    print("oracle/_ref: %d reference modules compiled into %s for Python %d.%d" % ((len(MODULES), OUT) + sys.version_info[:2]))


if __name__ == "__main__":
    main()
