"""The document splitter: LayoutLMv3 sequence classification of every page of a multi-page scan, from the page image, the OCR
words and their boxes; the label of a page says where a new document begins.

reference: ``BaseDocumentSplitter`` (marie/components/document_splitter/base.py:11-63) and ``TransformersDocumentSplitter``
(marie/components/document_splitter/transformers.py:30-229), whose image processor is
``LayoutLMv3ImageProcessor(apply_ocr=False, do_resize=True, resample=Image.LANCZOS)`` (:111-113).

The tokeniser, the weight loader and the model call are the document classifier's (``LayoutLMv3PagePredictor`` of
``document_classifier.py``); what differs is the LANCZOS page resize (Pillow-exact, in HIP: csrc/pil_resize.hip), the tag
(``tags["split"]``) and the absence of the ``task`` and ``top_k`` options.

Deliberate deviation: the reference's ``predict`` zips every batch against the whole ``words`` / ``boxes`` lists
(transformers.py:153), so the pages after the first batch are paired with the first pages' words.  Here page i gets
``words[i]`` and ``boxes[i]``.  There is no CPU path: ``use_gpu=False`` raises.
"""
from __future__ import annotations

import logging
from abc import ABC, abstractmethod
from typing import Dict, List, Optional, Union

import numpy as np

from ._lib import Context
from .document_classifier import LayoutLMv3PagePredictor
from .layoutlmv3 import PIL_LANCZOS


class BaseDocumentSplitter(ABC):
    """marie/components/document_splitter/base.py:11-63."""

    def __init__(self, **kwargs) -> None:
        self.logger = logging.getLogger(self.__class__.__name__)

    @abstractmethod
    def predict(self, documents, words: Optional[List[List[str]]] = None, boxes: Optional[List[List[List[int]]]] = None,
                batch_size: Optional[int] = None):
        """Predict the split labels of ``documents``."""

    def run(self, documents, words: Optional[List[List[str]]] = None, boxes: Optional[List[List[List[int]]]] = None,
            batch_size: Optional[int] = None):
        """base.py:36-63: ``predict`` on the documents; an empty list for none."""
        if documents:
            results = self.predict(documents=documents, words=words, boxes=boxes, batch_size=batch_size)
        else:
            results = []
        self.logger.info("Split documents with IDs: %s", [getattr(document, "id", None) for document in documents])
        return results


class TransformersDocumentSplitter(LayoutLMv3PagePredictor, BaseDocumentSplitter):
    """marie/components/document_splitter/transformers.py:30-229.  ``model_name_or_path`` is a local directory (see
    :class:`LayoutLMv3PagePredictor`); ``model_version``, ``use_auth_token`` and ``devices`` belong to the model hub and to
    torch device selection and are accepted for the signature only.  ``labels`` is kept, as in the reference, and like there
    the label names come from the model's ``id2label``.

    ``predict(documents, words, boxes, batch_size)`` sets ``tags["split"] = {"label", "score", "details"}`` on documents with
    ``.tensor`` and ``.tags`` (or returns these dictionaries for plain frames); ``predict_document_image(image, words, boxes,
    top_k)`` returns the one-entry list ``[{"label", "score"}]`` of a page (transformers.py:177-229)."""

    TAG = "split"
    RESAMPLE = PIL_LANCZOS

    def __init__(self, model_name_or_path: str, model_version: Optional[str] = None, tokenizer: Optional[str] = None,
                 use_gpu: bool = True, labels: Optional[List[str]] = None, batch_size: int = 16,
                 use_auth_token: Optional[Union[str, bool]] = None, devices: Optional[list] = None,
                 show_error: Optional[Union[str, bool]] = True, *, state: Optional[Dict[str, np.ndarray]] = None,
                 config: Optional[dict] = None, precision: str = "f16", ctx: Optional[Context] = None, **kwargs):
        super().__init__(**kwargs)
        self.show_error, self.labels = show_error, labels
        self._setup(model_name_or_path, tokenizer, use_gpu, batch_size, None, state, config, precision, ctx)
