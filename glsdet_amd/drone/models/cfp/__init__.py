"""Twinned modules live here; anything else of this package resolves to the reference checkout behind this drop-in
root on sys.path (the twins, found first, win)."""
import pkgutil

__path__ = pkgutil.extend_path(__path__, __name__)
