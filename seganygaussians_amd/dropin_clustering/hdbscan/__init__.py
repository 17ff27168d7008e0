"""`import hdbscan` for the reference's callers (saga_gui.py:529, the notebook's clustering cells): HDBSCAN(...).fit_predict on the
MI355X.  On sys.path only after seganygaussians_amd.install_dropin(fuse_clustering=True); a real `hdbscan` package is never
shadowed otherwise.  Euclidean only -- see seganygaussians_amd/clustering.py for the conventions and for the Jaccard path."""
from seganygaussians_amd.clustering import HDBSCAN  # noqa: F401

__all__ = ["HDBSCAN"]
