#!/usr/bin/env python
"""Same path and command line as funcwj/setk's scripts/sptk/rir_generate_1d.py;
the image method runs on the MI355X (setk_amd/sptk/rir_generate_1d.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from setk_amd.sptk.rir_generate_1d import main  # noqa: E402

if __name__ == "__main__":
    main()
