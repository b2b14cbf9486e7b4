"""Child process of tests/test_gpu_gap_variants.py: the library named by LNR_LIB (read when linear_amd.api is imported) filters the variant
inputs and writes the cords to an .npz:  python tests/gap_variant_child.py <out.npz>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out):
    from linear_amd import Filter, api
    from tests import gap_pool, gap_variant_inputs as vi
    assert os.environ.get("LNR_LIB") and os.path.samefile(api.SO, os.environ["LNR_LIB"])
    res = {}

    def run(tag, refs, T, reads, off, g, d, ext):
        f = Filter(device=0, gap_len=g, dup=d)
        try:
            f.build_index(refs, T)
            if ext:
                assert f.gap_stream(1) == 1
            coff, cs, ce = f.filter_batch(reads, off)
            res[tag + "_off"], res[tag + "_str"], res[tag + "_end"] = np.array(coff), np.array(cs), np.array(ce)
            res[tag + "_ext"] = np.array(f.gap_stream())
            res[tag + "_second"] = np.array(f.stats()["gap_second_pass"])
        finally:
            f.close()
    for name in vi.GOLDENS:
        refs, reads, off = vi.golden_inputs(name)
        for d in (0, 1):
            run(f"golden_{name}_dup{d}", refs, 1, reads, off, 50, d, 0)
    refs, reads, off = vi.sv_inputs()
    for g, d in vi.SV_MODES:
        run(f"sv_g{g}_dup{d}", refs, 1, reads, off, g, d, 0)
    P = gap_pool.make_pool()
    reads, off = gap_pool.pack(P.reads)
    for g, d in gap_pool.MODES:
        run(f"pool_g{g}_dup{d}", P.refs, P.T, reads, off, g, d, 1)
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
