"""Child program of tests/test_hip_inpaint_chain.py (started through tests/_variant_children.py: run_child): the shipped filter publisher
with the Inpainting method "telea_fronts" on the start state at cell_n 34, in a process of its own because EMAP_PLUGIN_RESIDENT is an
environment switch.  Writes the layers, their names and the route of each plugin layer into the .npz named on the command line."""
import os
import sys
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def main(out):
    import _inpaint_chain_cases as ic
    import _plug_cases as pc
    m = ic.twins(34, ic.CORE_FRONTS, Path(os.path.dirname(out)) / "child.yaml")
    m[1].close()
    names, got = m[0].get_grid_map_layers(pc.FILTER_PUBLISHER, order="message")
    route = m[0].last_plugin_route
    np.savez(out, layers=got, names=np.array(names), route=np.array([route[n] for n in names if n in route]))
    m[0].close()


if __name__ == "__main__":
    main(sys.argv[1])
