"""Drop-in check against the reference's OWN glue: with lgu_slam_amd's drop-in modules installed, the names the
reference's droid_slam/modules/corr.py and droid_slam/gaussianMask_cuda.py import and call resolve to this library's
operators, and the classes they offer have this build's counterparts with the same constructor parameters.  What the
reference imports, calls and offers is recorded in tests/golden/glue_surface.json (names only; written by
oracle/gen_glue_golden.py from the reference's modules)."""
import importlib
import inspect
import json
import os

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_reference_glue_imports_against_dropins(lgu):
    with open(os.path.join(GOLD, "glue_surface.json")) as fh:
        surface = json.load(fh)
    d, b = lgu.install_dropins()
    dropins = {"defCorrSample": d, "droid_backends": b}
    for name, mod in dropins.items():
        assert importlib.import_module(name) is mod     # `import defCorrSample` in the reference binds to the drop-in
    for module, rec in surface.items():
        assert rec["resolves"] and set(rec["resolves"]) <= set(dropins), module
        for ext, funcs in rec["resolves"].items():
            for f in funcs:
                assert callable(getattr(dropins[ext], f, None)), "%s: %s.%s" % (module, ext, f)
    # the names the reference glue resolves at call time are this library's functions
    assert d.defCorr_index_forward is lgu.ops.defCorr_index_forward
    assert b.altcorr_forward is lgu.ops.altcorr_forward
    # same public surface as this build's counterparts
    corr, ga = surface["modules.corr"], surface["gaussianMask_cuda"]
    for name in corr["public"]:
        assert hasattr(lgu.corr, name), name
    for name in ga["public"]:
        assert hasattr(lgu.gaussian_mask, name), name
    assert list(inspect.signature(lgu.CorrBlock.__init__).parameters) == corr["CorrBlock.__init__"]
    assert list(inspect.signature(lgu.AltCorrBlock.__init__).parameters) == corr["AltCorrBlock.__init__"]
    # identical parameter names -> a reference state dict loads into this build's GaussianMask
    assert sorted(dict(lgu.GaussianMask(4, 4).named_parameters())) == ga["GaussianMask(4, 4).named_parameters"]
