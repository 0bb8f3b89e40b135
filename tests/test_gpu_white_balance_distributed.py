"""Auto white balance over two ranks through the HIP kernels (both on cuda:0, fresh child processes, gloo for the
pending rows): every rank's ISP gathers the statistics of its own frames, the update all-gathers the ranks' rows and sums
them, so both ranks hold identical gains, equal to the contract over the union of their frames."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import isp_oracle as O
from tests import awb_ref as A
from tests.test_gpu_shading import raw_x

pytestmark = pytest.mark.gpu

H, W = 64, 128
STEPS = 3
WB = np.array([1.8, 1.0, 2.1])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _codes(step, k):
    rng = np.random.default_rng(100 * step + k)
    cast = [(1.0, 0.8, 0.6), (0.7, 0.9, 1.0), (0.9, 0.8, 0.9)][(step + k) % 3]
    base = 0.05 + 0.9 * rng.random((H, W, 1))
    img = np.clip(base * np.array(cast)[None, None, :], 0, 1).astype(np.float32)
    return np.rint(O.rgb_to_bayer(img, O.GRBG).astype(np.float64) * 4095).astype(np.uint16)


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import taichi_image_amd as ti
    isp = ti.Camera16(ti.BayerPattern.GRBG, moving_alpha=0.3, device=dev, process_group=dist.group.WORLD,
                      auto_white_balance=True)
    out = []
    for step in range(STEPS):
        frames = [torch.from_numpy(O.encode12(_codes(step, k))).to(dev) for k in range(4)][rank::world]
        isp.tonemap_reinhard(isp.load_packed12_batch(frames))
        out.append(isp.white_balance_gains.cpu().numpy())
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_share_one_white_balance():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    st = A.State(WB)
    for step in range(STEPS):
        st.update(A.add(*[A.stats(raw_x(_codes(step, k), 12, None, None)) for k in range(4)]), O.GRBG, 0.3)
        for r in range(world):
            assert np.array_equal(got[r][step], st.gains), (step, r, got[r][step], st.gains)
    assert not np.array_equal(st.gains, WB.astype(np.float32))
