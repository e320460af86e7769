"""The reference's real route to several GPUs (experiments/train_1d_edm.py:34-41,65-70): Lightning wraps the module in
``torch.nn.parallel.DistributedDataParallel`` and calls ``loss.backward()``.  Two ranks (RCCL when the box has >= 2 GPUs, otherwise
both on cuda:0 over gloo) wrap ``tqdne_amd.LightningEDM`` in torch's DDP -- default options, ``gradient_as_bucket_view=True``,
``static_graph=True`` (Lightning's defaults differ by version) and many small buckets -- and must reproduce the one-rank full-batch
gradients and Adam steps.  The worker is tests/_torch_ddp_worker.py."""

import pytest

from _ddp_launch import run_ranks

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(900)
def test_torch_ddp_wrapper_reproduces_full_batch_gradients_and_steps():
    res = run_ranks("_torch_ddp_worker.py", timeout=800, tag="TORCH_DDP_RESULT")
    assert set(res) == {"default", "bucket_view", "static_graph", "small_buckets"}
    for mode, r in res.items():
        # (the B = 4 per-rank plan and the B = 8 one-rank plan associate the GroupNorm / weight-gradient sums differently: 1e-5 on
        # the flat vector, the per-tensor figure is against each tensor's own largest entry)
        assert r["err_flat"] < 1e-5 and r["err_worst_tensor"] < 5e-4, (mode, r)
        assert r["replicas_equal"], mode
        assert abs(r["loss_mean"] - r["loss_full"]) < 1e-5 * abs(r["loss_full"]), (mode, r)
        assert r["weights_vs_full"] < 0.01, (mode, r)   # fraction of weights further than 1e-5 from the one-rank run's after two Adam steps
