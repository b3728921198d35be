"""Host-side pieces of the DLRM inference path (no GPU): the flag surface, the chunked 16-bit table cast and the latency
bookkeeping of --mode inference_benchmark (Recommendation/DLRM/dlrm/scripts/main.py:284-320, 524-541)."""
import pytest
import torch

from deeplearningexamples_amd.dlrm import infer as I
from deeplearningexamples_amd.dlrm.main import parse_flags


def test_inference_benchmark_flags_parse():
    f = parse_flags(["--mode", "inference_benchmark", "--dataset_type", "synthetic_gpu"])
    assert f.mode == "inference_benchmark"
    assert f.inference_benchmark_batch_sizes == [1, 64, 4096] and f.inference_benchmark_steps == 200
    g = parse_flags(["--mode", "inference_benchmark", "--dataset_type", "synthetic_gpu", "--inference_benchmark_batch_sizes", "2,8",
                     "--inference_benchmark_steps", "14", "--cuda_graphs", "--amp"])
    assert g.inference_benchmark_batch_sizes == [2, 8] and g.inference_benchmark_steps == 14 and g.cuda_graphs and g.amp


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("rows,chunk", [(1000, 256), (1000, 333), (7, 8), (512, 512), (1, 1)])
def test_chunked_cast_matches_one_cast(dtype, rows, chunk):
    g = torch.Generator().manual_seed(rows + chunk)
    w = torch.randn((rows, 24), generator=g) * 3.0
    w[0, 0], w[-1, -1] = 1.0 + 2.0 ** -11, 70000.0          # an fp16 tie, an fp16 overflow
    got = I.cast_table_chunked(w, dtype, chunk_rows=chunk)
    assert got.dtype == dtype and got.shape == w.shape
    assert torch.equal(got.view(torch.int16), w.to(dtype).view(torch.int16))


class _StubPredictor:
    def __init__(self):
        self.calls = 0

    def __call__(self, num, cat):
        self.calls += 1
        return torch.full((num.shape[0], 1), float(self.calls))


def test_latency_bookkeeping():
    """Steps 0 .. num_batches inclusive run (`if step > num_batches: break`), the latencies of steps >= warm-up are kept, the first
    10 of those are dropped, and the record holds mean latency and batch / mean latency under the reference's key names."""
    bs, ticks = 4, iter(range(1000))
    clock = lambda: float(next(ticks) ** 2)                   # latency of call k (from 0): (2k+1)^2 - (2k)^2 = 4k + 1
    batches = [(torch.zeros(bs, 3), torch.zeros(bs, 2, dtype=torch.int64), torch.ones(bs))] * 100
    stub, syncs = _StubPredictor(), []
    lat, y_true, y_score = I.benchmark_latencies(stub, batches, 14, warmup_steps=2, synchronize=lambda: syncs.append(1), clock=clock)
    assert stub.calls == 15 and len(syncs) == 15 and len(y_true) == 15 and len(y_score) == 15
    assert lat == [4.0 * k + 1 for k in range(2, 15)]
    assert y_score[3].shape == (bs,) and float(y_score[3][0]) == 4.0
    rec = I.summarize_latencies(lat, bs)
    kept = lat[10:]
    mean = sum(kept) / len(kept)
    assert rec == {"mean_inference_latency_batch_4": mean, "mean_inference_throughput_batch_4": bs / mean}
    with pytest.raises(ValueError):
        I.summarize_latencies(lat[:10], bs)
