#!/usr/bin/env python
"""Same path and command line as funcwj/setk's scripts/sptk/estimate_cacgmm_masks.py;
the EM runs on the MI355X (setk_amd/sptk/estimate_cacgmm_masks.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from setk_amd.sptk.estimate_cacgmm_masks import main  # noqa: E402

if __name__ == "__main__":
    main()
