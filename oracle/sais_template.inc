/* TEST INFRASTRUCTURE -- CPU oracle, not product code.
 *
 * Cyclic SA-IS ("BWT without sentinel"), restated from the reference:
 *   src/suffix_array/sais.rs:70-264   (fill, induce_sa, sa_is)
 *   src/suffix_array/ls_type.rs:10-92 (LSTypeArray::with_shift)
 *   src/suffix_array/bucket.rs:18-85  (BucketBuilder / Bucket)
 *
 * This file is a poor man's generic: it is included twice by bz2_oracle.c, once
 * with SA_T = uint8_t (the block bytes) and once with SA_T = size_t (the names
 * of the reduced problem, sais.rs:224).  SA_NAME(x) decorates the symbols.
 *
 * Data-structure restatements:
 *   LSTypeArray.bitmap / .is_lms  -> two byte arrays (one byte per flag)
 *   BucketBuilder.data            -> size_t array of (max-min+2) exclusive sums
 *   Bucket                        -> a working copy of starts or ends, indexed
 *                                    through the character at a text position
 */

#ifndef SA_T
#error "define SA_T and SA_NAME before including"
#endif

/* ls_type.rs:10-79 */
static void SA_NAME(ls_types)(const SA_T *array, size_t count, size_t shift,
                              uint8_t *bitmap, uint8_t *is_lms)
{
    memset(bitmap, 0, count);
    size_t start = (shift == 0) ? count : shift;

    /* ls_type.rs:21-31 */
    for (size_t i = start; i-- > 1;) {
        uint8_t b = bitmap[i];
        bitmap[i - 1] = (array[i] == array[i - 1]) ? b
                                                   : (uint8_t)(array[i - 1] < array[i]);
    }

    /* ls_type.rs:33-54 */
    if (shift != 0) {
        uint8_t b0 = bitmap[0];
        bitmap[count - 1] = (array[0] == array[count - 1])
                                ? b0
                                : (uint8_t)(array[count - 1] < array[0]);
        for (size_t i = count; i-- > shift + 1;) {
            uint8_t b = bitmap[i];
            bitmap[i - 1] = (array[i] == array[i - 1])
                                ? b
                                : (uint8_t)(array[i - 1] < array[i]);
        }
    }

    /* ls_type.rs:56-77 */
    if (shift == 0) {
        uint8_t old = 1;
        for (size_t i = 0; i < count; i++) {
            uint8_t b = bitmap[i];
            is_lms[i] = (uint8_t)(b && !old);
            old = b;
        }
    } else {
        uint8_t old = bitmap[count - 1];
        for (size_t i = 0; i < count; i++) {
            uint8_t b = bitmap[i];
            is_lms[i] = (uint8_t)(i != shift && b && !old);
            old = b;
        }
    }
}

/* bucket.rs:18-38: exclusive prefix sums of the character counts */
static size_t *SA_NAME(bucket_builder)(const SA_T *array, size_t count,
                                       size_t min, size_t max)
{
    size_t len = max - min + 2;
    size_t *data = (size_t *)calloc(len, sizeof(size_t));
    for (size_t i = 0; i < count; i++) {
        size_t v = (size_t)array[i];
        if (v > max || v < min) {
            fprintf(stderr, "oracle: bucket value out of range\n");
            abort(); /* bucket.rs:23-28 panics */
        }
        data[v - min] += 1;
    }
    size_t sum = 0;
    for (size_t i = 0; i < len; i++) {
        size_t val = data[i];
        data[i] = sum;
        sum += val;
    }
    return data;
}

/* bucket.rs:40-53: has_end -> bucket ends (exclusive), else bucket starts */
static void SA_NAME(bucket_build)(const size_t *builder, size_t len /* max-min+2 */,
                                  int has_end, size_t *out /* len-1 */)
{
    for (size_t i = 0; i + 1 < len; i++)
        out[i] = has_end ? builder[i + 1] : builder[i];
}

/* sais.rs:76-121 */
static void SA_NAME(induce_sa)(const SA_T *array, size_t count, size_t min,
                               const size_t *builder, size_t blen,
                               const uint8_t *types, size_t *sa, size_t shift)
{
    size_t *bucket = (size_t *)malloc((blen - 1) * sizeof(size_t));
#define BKT(pos) bucket[(size_t)array[(pos)] - min]
    /* compute SAl (sais.rs:85-105) */
    {
        SA_NAME(bucket_build)(builder, blen, 0, bucket);
        size_t k = ((shift == 0) ? count : shift) - 1; /* the "sentinel" position */
        size_t bk = BKT(k);
        sa[bk] = k;
        BKT(k) = bk + 1;

        for (size_t i = 0; i < count; i++) {
            size_t j = sa[i];
            if (j < SIZE_MAX && j != shift) {
                j = ((j == 0) ? count : j) - 1;
                if (!types[j]) {
                    size_t bj = BKT(j);
                    sa[bj] = j;
                    BKT(j) = bj + 1;
                }
            }
        }
    }
    /* compute SAs (sais.rs:107-120) */
    {
        SA_NAME(bucket_build)(builder, blen, 1, bucket);
        for (size_t i = count; i-- > 0;) {
            size_t j = sa[i];
            if (j < SIZE_MAX && j != shift) {
                j = ((j == 0) ? count : j) - 1;
                if (types[j]) {
                    size_t bj = BKT(j) - 1;
                    BKT(j) = bj;
                    sa[bj] = j;
                }
            }
        }
    }
#undef BKT
    free(bucket);
}

#ifndef SA_RECURSE_DECLARED
#define SA_RECURSE_DECLARED
static void sais_usize_sa_is(const size_t *array, size_t count, size_t *sa,
                             size_t bucket_min, size_t bucket_max, size_t shift);
#endif

/* sais.rs:127-264 */
static void SA_NAME(sa_is)(const SA_T *array, size_t count, size_t *sa,
                           size_t bucket_min, size_t bucket_max, size_t shift)
{
    uint8_t *types = (uint8_t *)malloc(count ? count : 1);
    uint8_t *lms = (uint8_t *)malloc(count ? count : 1);
    SA_NAME(ls_types)(array, count, shift, types, lms);

    /* stage 1 (sais.rs:139-155) */
    size_t blen = bucket_max - bucket_min + 2;
    size_t *builder = SA_NAME(bucket_builder)(array, count, bucket_min, bucket_max);
    size_t *bucket = (size_t *)malloc((blen - 1) * sizeof(size_t));
#define BKT(pos) bucket[(size_t)array[(pos)] - bucket_min]
    SA_NAME(bucket_build)(builder, blen, 1, bucket);

    for (size_t i = 0; i < count; i++) sa[i] = SIZE_MAX;

    /* for i in ((shift + 1)..count).chain(0..shift) */
    for (size_t pass = 0; pass < 2; pass++) {
        size_t lo = pass == 0 ? shift + 1 : 0;
        size_t hi = pass == 0 ? count : shift;
        for (size_t i = lo; i < hi; i++) {
            if (lms[i]) {
                size_t bi = BKT(i) - 1;
                BKT(i) = bi;
                sa[bi] = i;
            }
        }
    }
    SA_NAME(induce_sa)(array, count, bucket_min, builder, blen, types, sa, shift);

    /* compact the sorted LMS substrings (sais.rs:157-166) */
    size_t n1 = 0;
    for (size_t i = 0; i < count; i++) {
        if (lms[sa[i]]) {
            sa[n1] = sa[i];
            n1 += 1;
        }
    }

    /* name the substrings (sais.rs:168-207) */
    for (size_t i = n1; i < count; i++) sa[i] = SIZE_MAX;
    size_t name = 0;
    size_t prev_store = SIZE_MAX;

    for (size_t i = 0; i < n1; i++) {
        size_t prev = prev_store;
        size_t pos = sa[i];
        size_t now = pos;
        int diff = 0;
        for (;;) {
            if (prev == SIZE_MAX || now == shift || prev == shift ||
                array[now] != array[prev] || types[now] != types[prev]) {
                diff = 1;
                break;
            } else if (now != pos && (lms[now] || lms[prev])) {
                break;
            }
            now = (now == count - 1) ? 0 : now + 1;
            prev = (prev == count - 1) ? 0 : prev + 1;
        }
        if (diff) {
            name += 1;
            prev_store = pos;
        }
        pos = ((pos > shift) ? pos - shift : pos + count - shift) >> 1;
        sa[n1 + pos] = name - 1;
    }
    /* sais.rs:208-216 */
    if (count > 0) {
        size_t j = count - 1;
        size_t top = j;
        for (size_t i = top + 1; i-- > n1;) {
            if (sa[i] < SIZE_MAX) {
                sa[j] = sa[i];
                j -= 1; /* wraps only if every slot was taken, never read again */
            }
        }
    }

    /* stage 2 (sais.rs:218-230): s1 aliases the tail of sa */
    size_t *s1 = sa + (count - n1);
    if (name < n1) {
        sais_usize_sa_is(s1, n1, sa, 0, name - 1, 0);
    } else {
        for (size_t i = 0; i < n1; i++) sa[s1[i]] = i;
    }

    /* stage 3 (sais.rs:232-263) */
    SA_NAME(bucket_build)(builder, blen, 1, bucket);
    {
        size_t j = 0;
        for (size_t pass = 0; pass < 2; pass++) {
            size_t lo = pass == 0 ? shift + 1 : 0;
            size_t hi = pass == 0 ? count : shift;
            for (size_t i = lo; i < hi; i++) {
                if (lms[i]) {
                    s1[j] = i;
                    j += 1;
                }
            }
        }
    }
    for (size_t i = 0; i < n1; i++) sa[i] = s1[sa[i]];
    for (size_t i = n1; i < count; i++) sa[i] = SIZE_MAX;
    for (size_t i = n1; i-- > 0;) {
        size_t j = sa[i];
        sa[i] = SIZE_MAX;
        size_t b2j = BKT(j) - 1;
        BKT(j) = b2j;
        sa[b2j] = j;
    }
#undef BKT
    SA_NAME(induce_sa)(array, count, bucket_min, builder, blen, types, sa, shift);

    free(bucket);
    free(builder);
    free(types);
    free(lms);
}

#undef SA_T
#undef SA_NAME
