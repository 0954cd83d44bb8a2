"""CPU: the `--nti_batch` switch of `p2p/test.py` and the grouping of a shard into UNet batches (`ief_amd.nti.groups_of`,
`pad_group`) that `NTI.null_optimization_batched` and `BatchedNullTextOptimizer.begin` apply."""
import importlib.util
import os
import sys

import pytest

from ief_amd.nti import groups_of, pad_group

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P2P = os.path.join(ROOT, "image-editing-framework_amd", "p2p")


@pytest.fixture(scope="module")
def driver():
    """p2p/test.py loaded the way `python test.py` finds its neighbours, under a private module name"""
    saved_path = list(sys.path)
    saved_mods = {k: sys.modules.pop(k) for k in ("_bootstrap", "edit_real", "test") if k in sys.modules}
    try:
        sys.path.insert(0, P2P)
        spec = importlib.util.spec_from_file_location("_host_p2p_test", os.path.join(P2P, "test.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path[:] = saved_path
        for k in ("_bootstrap", "edit_real", "test"):
            sys.modules.pop(k, None)
        sys.modules.update(saved_mods)
    return mod


def test_nti_batch_flag_parses(driver):
    assert driver.parse_args([]).nti_batch == 1                      # default: today's path
    args = driver.parse_args(["--inversion_type", "null-text", "--nti_batch", "4", "--in_flight", "2", "--invert_batch", "4"])
    assert (args.nti_batch, args.in_flight, args.invert_batch, args.inversion_type) == (4, 2, 4, "null-text")
    import inspect
    assert inspect.signature(driver.run_items).parameters["nti_batch"].default == 1


@pytest.mark.parametrize("version", ["xl-base", "smallxl"])
def test_nti_batch_with_sdxl_is_an_argparse_error(driver, version, capsys):
    with pytest.raises(SystemExit) as e:
        driver.parse_args(["--sd_version", version, "--inversion_type", "null-text", "--nti_batch", "2"])
    assert e.value.code == 2 and "--nti_batch" in capsys.readouterr().err
    assert driver.parse_args(["--sd_version", version, "--inversion_type", "null-text"]).nti_batch == 1
    with pytest.raises(SystemExit):
        driver.parse_args(["--nti_batch", "0"])
    # the versions `_bootstrap._build_pipe` sends to `StableDiffusionXLPipeline`
    assert 'if sd_version in ("xl-base", "smallxl"):' in open(os.path.join(P2P, "_bootstrap.py")).read()
    assert driver.XL_VERSIONS == ("xl-base", "smallxl")


def test_grouping_and_padding_of_a_five_item_shard():
    assert groups_of(5, 2) == [[0, 1], [2, 3], [4]]
    assert [pad_group(g, 2) for g in groups_of(5, 2)] == [[0, 1], [2, 3], [4, 4]]
    assert groups_of(5, 4) == [[0, 1, 2, 3], [4]]
    assert [pad_group(g, 4) for g in groups_of(5, 4)] == [[0, 1, 2, 3], [4, 4, 4, 4]]
    assert pad_group([7, 8, 9], 4) == [7, 8, 9, 9]                    # copies of the LAST image
    assert groups_of(4, 4) == [[0, 1, 2, 3]] and groups_of(0, 4) == [] and groups_of(3, 1) == [[0], [1], [2]]
    for bad in ([], [1, 2, 3]):
        with pytest.raises(ValueError):
            pad_group(bad, 2)
    with pytest.raises(ValueError):
        groups_of(5, 0)
