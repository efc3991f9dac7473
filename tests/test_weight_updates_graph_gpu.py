"""GPU: ``ClipRunner(graph=True).submit`` after a weight update.  A captured step replays launches whose arguments are the tensors
the fused routes had derived from the weights at capture time (folded BN, transformed filters, stacked projections); the slot
remembers models.fused.derived_key of every parameter and buffer and is captured again when it has moved, and ``refresh()`` is
for the edits no key can see.  The geometry is the one test_clip_pipeline_submit_matches_call captures: one lane, 4 frames of
64 x 96, one process, no collective."""
import pytest
import torch

from tests import _lifecycle as L

pytestmark = pytest.mark.gpu


def _outputs(out):
    return [out["pred_logits"], out["pred_boxes"]] + list(out["topk"])


def _update_every_parameter_in_place(model):
    """The ``inplace`` kind (x 1.25 + 0.01, tests/_lifecycle.py) on every parameter - except that the 53 convolution weights of
    the ResNet body are scaled only.  A shift of 0.01 on ALL of them at once is a gain of 0.01 x fan-in (up to 46) per layer on
    the mean of the map: measured on the CPU with this model and clip, the stage maxima then run 6.2, 6.6e3, 6.8e10, 1.6e26,
    8.2e35 and the input projection's GroupNorm returns NaN, which compares unequal to itself.  Scaled only they run 6.2, 15,
    31, 93, 113 and every output stays finite (asserted).  Every parameter still changes in place, version counter bumped."""
    body = {id(p) for p in model.backbone[0].body.parameters()}
    with torch.no_grad():
        for p in model.parameters():
            if id(p) in body:
                p.mul_(1.25)
            else:
                p.mul_(1.25).add_(0.01)


def test_graph_replays_follow_weight_updates_and_capture_only_then(monkeypatch):
    from models.clip_inference import ClipRunner
    from tests.test_clip_shard_gpu import _build
    captures, real = [], ClipRunner._capture_slot

    def counting(self, *a, **k):
        captures.append(1)
        return real(self, *a, **k)

    monkeypatch.setattr(ClipRunner, "_capture_slot", counting)
    model = _build()
    clips = [torch.randn(4, 4, 64, 96, generator=torch.Generator().manual_seed(40 + i)).cuda() for i in range(2)]
    saved = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True         # see test_two_stream_schedule_gives_identical_outputs
    try:
        runner = ClipRunner(model, micro_batch=4, lanes=1, graph=True)

        def submits():
            outs = []
            for c in clips:
                out, done = runner.submit(c)
                done.synchronize()
                outs.append([t.clone() for t in _outputs(out)])
            return outs

        def fresh_eager():
            fresh = _build()
            fresh.load_state_dict(model.state_dict())
            eager = ClipRunner(fresh, micro_batch=4)
            return [[t.clone() for t in _outputs(eager(c))] for c in clips]

        first = submits()                              # captures on the first clip, replays on the second
        assert len(captures) == 1 and all(runner._graph_slots.values())

        _update_every_parameter_in_place(model)
        second = submits()
        assert len(captures) == 2
        assert all(torch.isfinite(t).all() for out in second for t in out if t.is_floating_point())
        for got, want, old in zip(second, fresh_eager(), first):
            L.assert_same(got, want, "replay after an in-place update of every parameter against a fresh eager runner")
            assert L.differs(got, old)

        L.apply_edit(model, "backbone.0.body.layer1.0.conv2", "weight", "data_inplace", runner=runner)
        third = submits()
        assert len(captures) == 3
        for got, want, old in zip(third, fresh_eager(), second):
            L.assert_same(got, want, "replay after p.data.mul_(), drop_derived and refresh against a fresh eager runner")
            assert L.differs(got, old)

        again = submits()                              # nothing changed: replays only
        assert len(captures) == 3
        for got, want in zip(again, third):
            L.assert_same(got, want, "replays with nothing in between")
    finally:
        torch.backends.cudnn.deterministic = saved
