"""marie_icr_amd: the document pipeline in HIP for gfx950.  The components live in their modules; the names below are
resolved on first use, so that importing the package loads nothing."""
__all__ = ["TransformersDocumentSplitter"]


def __getattr__(name):
    if name == "TransformersDocumentSplitter":
        from .document_splitter import TransformersDocumentSplitter

        return TransformersDocumentSplitter
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
