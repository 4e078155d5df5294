#!/usr/bin/env python
"""Same path and command line as funcwj/setk's scripts/sptk/wav_separate.py;
the computation runs on the MI355X (setk_amd/sptk/wav_separate.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from setk_amd.sptk.wav_separate import main  # noqa: E402

if __name__ == "__main__":
    main()
