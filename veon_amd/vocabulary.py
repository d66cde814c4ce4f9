"""The vocabulary lists of the open-vocabulary path: ``prepare_vocabulary`` +
``_add_vocabulary_nuscenes`` of the reference's entry module
(mmdet3d/models/semantic_net/san_in_veon_entry_temporal.py:94-112, 243-262).

The reference classifies against the DETAILED descriptions of its vocabulary ("car",
"sedan", "hatch-back", ...), keeps for every description the class it belongs to
(``class_reflection``) and merges the descriptions of one class by their maximum
(``occ_eval.occ_labels_grouped``).  The category lists themselves are data of the
caller: this package holds none.

The merge rule has one home here, for the kernels' wrappers and their torch mirrors alike:
``group_ids`` (runs of ``class_reflection`` -> merged classes), ``group_table`` (the
checked table the grouped tails take), ``merge_runs`` (the maximum over each run of rows)
and ``lowest_argmax`` (the tie-break).
"""
import torch

MAX_ROWS = 256       # logit rows of the grouped tails
MAX_MERGED = 64      # merged channels


def group_ids(class_reflection):
    """Merged class of every 2-D class: consecutive equal values of ``class_reflection``
    form one merged class, numbered in order of appearance -> (list, count)."""
    ref = [int(v) for v in class_reflection]
    gid, cur = [], -1
    for i, v in enumerate(ref):
        if i == 0 or v != ref[i - 1]:
            cur += 1
        gid.append(cur)
    return gid, cur + 1


def group_table(group, n_merged, free_label, K=None, with_hist=False):
    """The checked group table of the grouped tails as a list of ints: ``group[c]`` is
    the merged channel of logit row c.  ValueError unless 1 <= K <= 256, 1 <= n_merged
    <= 64, every entry is in [0, n_merged), the rows of a channel are consecutive (no
    split runs), no channel is used by two runs and every channel is used, and 0 <=
    free_label <= 255 (<= 63 with a histogram, whose side is max(n_merged, free_label +
    1))."""
    group = [int(v) for v in group]
    n_merged, free_label = int(n_merged), int(free_label)
    if K is not None and len(group) != K:
        raise ValueError('the group table has %d entries for %d logit rows' % (len(group), K))
    if not 1 <= len(group) <= MAX_ROWS:
        raise ValueError('the grouped tail takes 1 to %d logit rows, got %d'
                         % (MAX_ROWS, len(group)))
    if not 1 <= n_merged <= MAX_MERGED:
        raise ValueError('n_merged must be in [1, %d], got %d' % (MAX_MERGED, n_merged))
    if not 0 <= free_label <= 255:
        raise ValueError('free_label must be in [0, 255], got %d' % free_label)
    if with_hist and max(n_merged, free_label + 1) > MAX_MERGED:
        raise ValueError('the histogram holds at most %d classes, free_label is %d'
                         % (MAX_MERGED, free_label))
    seen = set()
    for c, ch in enumerate(group):
        if not 0 <= ch < n_merged:
            raise ValueError('row %d names merged channel %d of %d' % (c, ch, n_merged))
        if c == 0 or ch != group[c - 1]:
            if ch in seen:
                raise ValueError('merged channel %d is used by two runs of rows (a split '
                                 'run, or a channel used twice)' % ch)
            seen.add(ch)
    if len(seen) != n_merged:
        raise ValueError('%d of the %d merged channels have no row' %
                         (n_merged - len(seen), n_merged))
    return group


def merge_runs(t, group, n_merged):
    """(B, K, ...) -> (B, n_merged, ...): the maximum over each run of rows of ``group``
    (``torch.max``: NaN propagates)."""
    merged = [None] * n_merged
    left = 0
    while left < len(group):
        right = left
        while right + 1 < len(group) and group[right + 1] == group[left]:
            right += 1
        merged[group[left]] = torch.max(t[:, left:right + 1], dim=1).values
        left = right + 1
    return torch.stack(merged, dim=1)


def lowest_argmax(merged):
    """(B, n, ...) -> ((B, ...) int64, (B, 1, ...)): the lowest channel that attains the
    maximum over dim 1 (n where none does: a NaN among them), and that maximum."""
    n = merged.shape[1]
    top = merged.max(dim=1, keepdim=True).values
    index = torch.arange(n, device=merged.device).view((1, n) + (1,) * (merged.dim() - 2))
    return torch.where(merged == top, index, torch.full_like(index, n)).amin(dim=1), top


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
