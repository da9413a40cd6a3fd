"""The two scikit-image calls the reference's file I/O makes, over PIL (see io.py)."""
