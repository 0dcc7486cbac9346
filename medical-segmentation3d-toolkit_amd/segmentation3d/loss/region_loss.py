"""Regions for region-based models: validation and the label -> region lookup table (the
reference knows exclusive classes only).

`regions` is a list of R label-id sets (1 <= R <= 16, ids 1..255, background 0 in none), e.g. BraTS: whole tumour {1, 2, 3},
tumour core {1, 3}, enhancing tumour {3}.  Regions may overlap, so a region-based network has one sigmoid output per region
instead of a soft-max over exclusive classes.  Bit r of `lut[l]` says whether label l belongs to region r; the device code
(evaluation counts) looks memberships up in that 256-word table.  `region_class_order` is the label inference writes for each
region when it composes the thresholded region probabilities back into a label map.
"""
MAX_REGIONS = 16


def check_regions(regions):
    """-> list of R sorted label-id lists; ValueError unless 1 <= R <= 16 and every region is a non-empty set of distinct
    integer ids in 1..255"""
    if regions is None or isinstance(regions, (str, bytes)) or not hasattr(regions, '__len__'):
        raise ValueError('regions must be a list of label-id lists, got {!r}'.format(regions))
    if not 1 <= len(regions) <= MAX_REGIONS:
        raise ValueError('between 1 and {} regions are supported, got {}'.format(MAX_REGIONS, len(regions)))
    out = []
    for k, region in enumerate(regions):
        if isinstance(region, (str, bytes)) or not hasattr(region, '__iter__'):
            raise ValueError('region {} must be a list of label ids, got {!r}'.format(k, region))
        ids = list(region)
        if not ids:
            raise ValueError('region {} is empty'.format(k))
        for l in ids:
            if isinstance(l, bool) or int(l) != l or not 1 <= int(l) <= 255:
                raise ValueError('region {}: label id {!r} is not an integer in 1..255'.format(k, l))
        ids = [int(l) for l in ids]
        if len(set(ids)) != len(ids):
            raise ValueError('region {} lists a label id twice: {}'.format(k, ids))
        out.append(sorted(ids))
    return out


def check_region_class_order(region_class_order, num_regions):
    """-> list of R ints in 1..127 (the label written for region r at inference; the mask is int8)"""
    if region_class_order is None or isinstance(region_class_order, (str, bytes)) or not hasattr(region_class_order, '__len__'):
        raise ValueError('region_class_order must be a list of {} label ids, got {!r}'.format(num_regions, region_class_order))
    order = list(region_class_order)
    if len(order) != num_regions:
        raise ValueError('region_class_order has {} entries for {} regions'.format(len(order), num_regions))
    for l in order:
        if isinstance(l, bool) or int(l) != l or not 1 <= int(l) <= 127:
            raise ValueError('region_class_order entry {!r} is not an integer in 1..127'.format(l))
    return [int(l) for l in order]


def region_lut(regions):
    """the 256-word table of the kernels: bit r of lut[l] is set iff label l is in region r (a list of Python ints)"""
    lut = [0] * 256
    for r, region in enumerate(check_regions(regions)):
        for l in region:
            lut[l] |= 1 << r
    return lut
