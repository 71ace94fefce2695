"""FlowLoader's refusals that depend on the arguments alone: each comes before the Generator is created (no GPU).  The
package's Generator is swapped for a callable that raises a sentinel; a refused option set must raise its ValueError and
never get that far, a valid one must."""
import pytest


class Reached(Exception):
    """the loader got as far as creating its Generator"""


@pytest.fixture
def loader(ofdg, monkeypatch):
    def generator(*args, **kw):
        raise Reached()
    monkeypatch.setattr(ofdg, "Generator", generator)
    return ofdg.FlowLoader


def refused(ofdg):
    import torch
    return [
        (dict(pack=dict(dtype=torch.float16)), "unknown pack"),
        (dict(spatial=dict(zoom=1.0), spatial_size=(48, 96)), "unknown range .zoom."),
        (dict(spatial=ofdg.SPATIAL_FLOWNET), "spatial_size"),
        (dict(crop=(48, 96), spatial=ofdg.SPATIAL_FLOWNET, spatial_size=(48, 96)), "does not combine with spatial"),
        (dict(objects=True, extras=("label0", "label1"), spatial=ofdg.SPATIAL_FLOWNET, spatial_size=(48, 96)), "unwarped"),
        (dict(objects=True, extras=("label0", "label1"), crop=(48, 96)), "uncropped"),
        (dict(photo=dict(gamma=1.0)), "unknown range .gamma."),
        (dict(erase=dict(size=3)), "unknown erase"),
        (dict(erase=dict(ofdg.ERASE_RAFT, mark_occ=True), extras=("flow1",)), "occlusion map"),
        (dict(erase=dict(ofdg.ERASE_RAFT, frames=(0, 1)), extras=("occ0", "occ1")), "flow1"),
        (dict(erase=dict(frames=(3,))), "frames"),
        (dict(boundaries=dict(labels=True, frames=(0, 1)), extras=("flow1", "label0")), "label1"),
        (dict(boundaries=dict(frames=(0, 1)), extras=("label0", "label1")), "flow1"),
        (dict(boundaries=dict(labels=False), extras=("label0",)), "min_step"),
        (dict(boundaries=dict(radius=4)), "min_step"),
        (dict(boundaries=dict(rad=4)), "unknown boundaries"),
        (dict(image_dtype=torch.uint8, extras=("flow1",)), "extras_compact"),
        (dict(objects=True), "label0"),
    ]


def test_refusals_come_before_the_generator(ofdg, loader):
    cases = refused(ofdg)
    assert len(cases) == 18
    for options, word in cases:
        with pytest.raises(ValueError, match=word):
            loader(**options)


def test_a_valid_option_set_reaches_the_generator(ofdg, loader):
    with pytest.raises(Reached):
        loader(photo=ofdg.PHOTO_FLOWNET)
