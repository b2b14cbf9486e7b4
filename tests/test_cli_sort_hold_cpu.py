"""CPU: the front-end's --sort-device-mem / --sort-host-mem against the test double of the device half (tests/stub_abi.cpp + the real reader
and writer, as tests/test_cli_sort_cpu.py builds it): either option without --sort is refused with a message that names it and --sort; a
SIZE that is not digits with an optional K, M or G is refused; with --sort and everything else the double has no GPU side, so the run is
refused for the missing device; the usage text lists both options."""
import pytest

from tests.test_cli_frontend_cpu import write_inputs
from tests.test_cli_sort_cpu import cli, outputs, run  # noqa: F401  (cli: the fixture that builds the double)


@pytest.mark.parametrize("opt", ["--sort-device-mem", "--sort-host-mem"])
def test_the_options_need_sort(cli, tmp_path, opt):  # noqa: F811
    reads, ref = write_inputs(tmp_path, n_reads=60)
    for form in ([opt, "64M"], [opt + "=64M"]):
        p = run(cli, ["filter", reads[0], ref, "-t", "2", "-ot", "4", "-o", str(tmp_path / "so"), "--gpu-writer"] + form, tmp_path)
        assert p.returncode == 1, p.stderr.decode()
        assert opt.encode() in p.stderr and b"needs --sort" in p.stderr
        assert outputs(tmp_path, "so") == []


@pytest.mark.parametrize("opt", ["--sort-device-mem", "--sort-host-mem"])
@pytest.mark.parametrize("size", ["12Q", "", "K", "1.5G", "-3", "12KK", "99999999999999999999G"])
def test_a_malformed_size(cli, tmp_path, opt, size):  # noqa: F811
    reads, ref = write_inputs(tmp_path, n_reads=60)
    p = run(cli, ["filter", reads[0], ref, "-t", "2", "-ot", "4", "-o", str(tmp_path / "so"), "--gpu-writer", "--sort", opt, size], tmp_path)
    assert p.returncode == 1, p.stderr.decode()
    assert opt.encode() in p.stderr and b"SIZE" in p.stderr and b"no usable device" not in p.stderr
    assert outputs(tmp_path, "so") == []


@pytest.mark.parametrize("size", ["0", "7", "64K", "64M", "3G"])
def test_well_formed_sizes_reach_the_device_check(cli, tmp_path, size):  # noqa: F811
    reads, ref = write_inputs(tmp_path, n_reads=60)
    p = run(cli, ["filter", reads[0], ref, "-t", "2", "-ot", "12", "-o", str(tmp_path / "so"), "--gpu-writer", "--sort", "--sort-device-mem", size, "--sort-host-mem=" + size], tmp_path)
    assert p.returncode == 1 and b"no usable device" in p.stderr, p.stderr.decode()
    assert outputs(tmp_path, "so") == []


def test_usage_lists_the_options(cli, tmp_path):  # noqa: F811
    p = run(cli, ["filter", "-h", "x", "y"], tmp_path)
    assert p.returncode == 0
    tail = p.stderr.split(b"MI355X front-end")[1]
    assert b"--sort-device-mem SIZE" in tail and b"--sort-host-mem SIZE" in tail and b"pinned host memory" in tail
