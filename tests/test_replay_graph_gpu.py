"""graphs.ReplayGraph on the device: a two-launch body on static buffers, replayed and re-captured, against the same two launches eager."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cover_vla_amd import graphs, ops  # noqa: E402


def test_replay_graph_follows_its_static_buffers_and_recaptures_on_a_moved_generation(dev, monkeypatch):
    """Body: ops.copy_rows of a bf16 [4, 64] source into a destination, then ops.scale_bf16 of the destination by 2 (exact in bf16).
    The source is refilled before every run(); after each the destination equals the eager two-launch result bit for bit: the eager
    first call, three replays, then -- the generation moved -- a call that captures again (counted at graphs.capture) and a replay."""
    real, captures = graphs.capture, []
    monkeypatch.setattr(graphs, "capture", lambda fn, device: (captures.append(1), real(fn, device))[1])
    rows, cols = 4, 64
    src, dst, ref = (torch.zeros(rows, cols, dtype=torch.bfloat16, device=dev) for _ in range(3))
    two_launches = lambda out: (ops.copy_rows(src, out, rows, cols), ops.scale_bf16(out, 1.0, 2.0))
    generation = [0]
    rg = graphs.ReplayGraph(lambda: two_launches(dst), dev, gen=lambda: generation[0])
    assert not rg.captured
    g = torch.Generator().manual_seed(3)
    for call in range(6):
        if call == 4:
            generation[0] = 1
        src.copy_(torch.randn(rows, cols, generator=g).to(torch.bfloat16))
        rg.run()
        two_launches(ref)
        torch.cuda.synchronize()
        assert torch.equal(dst.view(torch.int16), ref.view(torch.int16)), call
        assert torch.equal(dst.float(), src.float() * 2) and bool(dst.any()), call
        assert rg.captured and rg.gen == (0 if call < 4 else 1)
        assert len(captures) == (1 if call < 4 else 2), call
