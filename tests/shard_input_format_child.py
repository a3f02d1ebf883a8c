"""Child process of tests/test_gpu_input_format.py: one step of the fovea shard (ugsm_submit_fovea_shard over a one-rank RCCL communicator,
joined as tests/rccl_shard_child.py joins it) on a BGR8 pair, against ugsm_submit_foveated on the pair's rgb8 conversion, bit for bit; and a
stride below 3 W refused with UGSM_ERR_SIZE_MISMATCH before anything is enqueued.  A process of its own: the torch.distributed group that hands
the id round must come first, and a hang inside RCCL must not take the test session with it.  Prints "SHARD_FORMAT_OK" on success."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

os.environ.setdefault("RANK", "0")
os.environ.setdefault("LOCAL_RANK", "0")
os.environ.setdefault("WORLD_SIZE", "1")
os.environ["UGSM_FORCE_DIST"] = "1"


def main():
    import numpy as np
    import torch
    import encode_np as en
    from ug_stereomatcher_amd import _lib, dist as ud, synth

    W, H, levels, F, off = 643, 481, 10, 5, (-37, 21)
    rank, local_rank, world = ud.init()  # before any other GPU call of this process
    assert world == 1
    dev = torch.device("cuda", local_rank)
    fw, fh = _lib.fovea_dims(W, H, levels, F)
    L, R, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 77)
    bgrL, bgrR = (torch.from_numpy(en.encode(a, en.BGR8)).to(dev) for a in (L, R))
    rgbL, rgbR = (torch.from_numpy(en.to_rgb8(en.encode(a, en.BGR8), en.BGR8)).to(dev) for a in (L, R))
    with _lib.Context(device=local_rank, levels=levels, fovea_levels=F, slots=1) as ctx:
        lib, h = ctx.lib, ctx.handle
        want = torch.empty((3, F, fh, fw), dtype=torch.float32, device=dev)
        ctx.check(lib.ugsm_submit_foveated(h, 0, rgbL.data_ptr(), rgbR.data_ptr(), W, H, 3 * W, off[0], off[1], want.data_ptr(), None, None))
        ctx.check(lib.ugsm_wait(h, 0))
        assert ud.shard_init(ctx, rank, world) == 1
        ctx.set_input_format(_lib.UGSM_INPUT_BGR8)
        got = torch.full((3, F, fh, fw), float("nan"), dtype=torch.float32, device=dev)
        st = lib.ugsm_submit_fovea_shard(h, 0, bgrL.data_ptr(), bgrR.data_ptr(), W, H, 3 * W - 1, off[0], off[1], got.data_ptr(), 0)
        assert st == _lib.UGSM_ERR_SIZE_MISMATCH, st
        ctx.check(lib.ugsm_submit_fovea_shard(h, 0, bgrL.data_ptr(), bgrR.data_ptr(), W, H, 3 * W, off[0], off[1], got.data_ptr(), 0))
        ctx.check(lib.ugsm_wait(h, 0))
        torch.cuda.synchronize()
        same = torch.equal(got.view(torch.int32), want.view(torch.int32))
        ctx.shard_finalize()
    if not same:
        raise SystemExit("the BGR8 shard step differs from the rgb8 foveated call on the conversion")
    print("SHARD_FORMAT_OK", np.int64(fw * fh * F))


if __name__ == "__main__":
    main()
