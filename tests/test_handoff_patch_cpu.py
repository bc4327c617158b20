"""handoff._Patch, the one patch-and-restore of the hand-off classes, on plain Python objects (no GPU, no torch modules)."""
import pytest

from x2i_amd.handoff import _Patch


class Model:
    def generate(self, x):
        return ("the class's", x)


def own(x):
    return ("the instance's", x)


def _run(case, m, patch):
    if case == "install and remove":
        assert patch.install() is patch and m.generate(1) == ("patched", 1)
        patch.remove()
    elif case == "context manager":
        with patch as p:
            assert p is patch and m.generate(1) == ("patched", 1)
    elif case == "exception inside with":
        with pytest.raises(KeyError):
            with patch:
                assert m.generate(1) == ("patched", 1)
                raise KeyError("inside")
    elif case == "install twice, remove twice":
        assert patch.install() is patch and patch.install() is patch and m.generate(1) == ("patched", 1)
        patch.remove()
        patch.remove()
        assert patch.install().install() is patch and m.generate(1) == ("patched", 1)       # and it can be installed again
        patch.remove()


@pytest.mark.parametrize("has_own", [False, True], ids=["absent from the instance", "the instance's own"])
@pytest.mark.parametrize("case", ["install and remove", "context manager", "exception inside with", "install twice, remove twice"])
def test_patch_replaces_an_attribute_on_the_instance_and_restores_it(case, has_own):
    m = Model()
    m.other = 3
    if has_own:
        m.generate = own
    before = dict(m.__dict__)
    bound = m.generate
    patch = _Patch(m, "generate", lambda x: ("patched", x))
    patch.remove()                                        # harmless before any install
    assert m.__dict__ == before
    _run(case, m, patch)
    assert m.__dict__ == before and ("generate" in m.__dict__) == has_own
    assert m.generate(2) == (("the instance's", 2) if has_own else ("the class's", 2))
    if has_own:
        assert m.generate is own and patch._original is own
    else:
        assert patch._original == bound and patch._original.__self__ is m         # the bound method from before
    assert patch._original(5) == bound(5)
    assert Model().generate(0) == ("the class's", 0)      # the class was never touched


def test_the_hand_off_classes_are_patches():
    from x2i_amd import handoff
    for cls in (handoff.HipVision, handoff.HipSiglip, handoff.HipResampler, handoff.HipAudio, handoff.HipInternVision, handoff._PromptHandoff):
        assert issubclass(cls, _Patch)
        assert all(name not in vars(cls) for name in ("install", "remove", "__enter__", "__exit__"))      # one copy, the helper's
