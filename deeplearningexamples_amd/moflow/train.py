"""Not built: training (the reference's moflow/runtime/train.py).  The generator (generate.py) is."""
import sys


def main(argv=None):
    raise SystemExit("MoFlow: training is not built in this project; molecule generation is "
                     "(python -m deeplearningexamples_amd.moflow.generate)")


if __name__ == "__main__":
    main(sys.argv[1:])
