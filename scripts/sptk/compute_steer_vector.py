#!/usr/bin/env python
"""Same path and command line as funcwj/setk's scripts/sptk/compute_steer_vector.py;
host only (setk_amd/sptk/compute_steer_vector.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from setk_amd.sptk.compute_steer_vector import main  # noqa: E402

if __name__ == "__main__":
    main()
