"""Not built: the metrics of the reference's moflow/runtime/evaluate.py (validity, uniqueness, novelty: rdkit and the training set).  The generator (generate.py) is."""
import sys


def main(argv=None):
    raise SystemExit("MoFlow: the metrics of the reference's moflow/runtime/evaluate.py are not built in this project; molecule generation is "
                     "(python -m deeplearningexamples_amd.moflow.generate)")


if __name__ == "__main__":
    main(sys.argv[1:])
