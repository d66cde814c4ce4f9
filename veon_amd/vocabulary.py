"""The vocabulary lists of the open-vocabulary path: ``prepare_vocabulary`` +
``_add_vocabulary_nuscenes`` of the reference's entry module
(mmdet3d/models/semantic_net/san_in_veon_entry_temporal.py:94-112, 243-262).

The reference classifies against the DETAILED descriptions of its vocabulary ("car",
"sedan", "hatch-back", ...), keeps for every description the class it belongs to
(``class_reflection``) and merges the descriptions of one class by their maximum
(``occ_eval.occ_labels_grouped``).  The category lists themselves are data of the
caller: this package holds none.
"""


def build_vocabulary(words, categories):
    """-> (vocabulary, detailed_description, class_reflection), three lists of one length.

    ``words``: the user's own class names; lower-cased and stripped, empty ones dropped,
    each of them a class of its own in front of the categories' classes.  ``categories``:
    a list of ``{"category": name, "detailed_items": [[brief] or [brief, detail], ...]}``
    (e.g. read from JSON); category i becomes class ``len(words) + i``, every item one
    entry: ``brief`` in the vocabulary, ``brief`` or ``brief, in detail 'detail'`` among
    the descriptions.  An item whose brief name the user already gave is left out, as in
    the reference.

    One departure, on purpose: the user's words are de-duplicated IN ORDER (first
    occurrence wins).  The reference's ``list(set(...))`` has no defined order, so for more
    than one word its class numbers change from run to run."""
    seen, vocabulary = set(), []
    for w in words:
        w = w.lower().strip()
        if w != '' and w not in seen:
            seen.add(w)
            vocabulary.append(w)
    detailed = list(vocabulary)
    reflection = list(range(len(vocabulary)))
    start = len(vocabulary)
    given = set(vocabulary)
    out_voc, out_det, out_ref = list(vocabulary), detailed, reflection
    for i, info in enumerate(categories):
        for item in info['detailed_items']:
            brief = item[0]
            if brief in given:
                continue
            out_voc.append(brief)
            out_det.append(brief if len(item) == 1
                           else brief + ", in detail '" + item[1] + "'")
            out_ref.append(start + i)
    return out_voc, out_det, out_ref
