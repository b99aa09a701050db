"""One rank of a two-rank job for tests/test_gpu_gmti.py: TwoChannelBatch(stack="detections") on the GPU with the stack gathered
through a gloo group (both ranks share the one GPU of the test box)."""
import os
import sys

import numpy as np
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conftest  # noqa: F401,E402
import sarx  # noqa: E402
from sarx.batch import TorchStackComm, TwoChannelBatch  # noqa: E402


def main():
    out, n, n_frames, max_det = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    dist.init_process_group("gloo")
    comm = TorchStackComm()
    ctx = sarx.Context(0)
    b = TwoChannelBatch(ctx, n, n_frames, comm.world, comm.rank, stack="detections", scene="c3", scene_scale=0.25, host_comm=comm,
                        detect=sarx.GmtiParams(max_detections=max_det))
    b.run()
    ctx.sync()
    whole = b.d_stack.download(np.float32, (b.n_rounds * comm.world, *b.slot_shape))      # pad slots included
    np.save(os.path.join(out, f"gmti_stack_rank{comm.rank}.npy"), whole)
    b.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
