/*
 * MatrixFactorizationSGD.java -- the Java host surface over libmfsgd.so.
 *
 * UNCOMPILED AND UNTESTED: neither this container nor the GPU box has a JDK
 * (javac/java absent, no jni.h), see DESIGN.md section 8.  The reference
 * repository contains no Java source either (/root/reference/README.md:1-2 is
 * all of it); the surface is the one BASELINE.json names -- a class
 * MatrixFactorizationSGD with train()/predict() -- with the parameter lists
 * SURVEY.md section 8b proposes.  Every native method is one call into the
 * C-ABI of include/mfsgd.h through jni/mfsgd_jni.cpp.
 */
public final class MatrixFactorizationSGD implements AutoCloseable {
    static {
        System.loadLibrary("mfsgd_jni"); // libmfsgd_jni.so, linked against libmfsgd.so
    }

    private long handle; // mfsgd_handle*
    private long ring;   // mfsgd_dsgd* (trainDistributed), 0 until the first call
    private int slots;   // item partitions this rank holds at a time (nParts / world)
    private int users, items; // follow the handle: addUsers / addItems grow them
    private final int k, nParts;
    private final long seed;
    private boolean initialised;

    public MatrixFactorizationSGD(int users, int items, int k, float lr, float lambda, long seed) {
        this.users = users;
        this.items = items;
        this.k = k;
        this.seed = seed;
        this.nParts = 1;
        this.handle = nativeCreate(users, items, k, lr, lambda, /*device*/ 0, /*nParts*/ 0);
    }

    /**
     * One rank of a DSGD job (one JVM process per GPU): this rank's {@code users} P rows, the GLOBAL item count, and
     * {@code nParts = world * partsPerRank} item partitions whose Q blocks travel round the ring of ranks.
     */
    public MatrixFactorizationSGD(int users, int items, int k, float lr, float lambda, long seed, int device, int nParts) {
        if (nParts < 2) throw new IllegalArgumentException("a distributed handle has at least two item partitions");
        this.users = users;
        this.items = items;
        this.k = k;
        this.seed = seed;
        this.nParts = nParts;
        this.handle = nativeCreate(users, items, k, lr, lambda, device, nParts);
    }

    /** Runs {@code epochs} SGD passes over the ratings; returns the RMSE after each epoch. */
    public double[] train(int[] u, int[] i, float[] r, int epochs) {
        if (u.length != i.length || u.length != r.length) throw new IllegalArgumentException("length mismatch");
        // The library recognises the same triples again (length + a 128-bit hash of every byte) and keeps
        // its schedules, so repeated train() calls on one rating set pay for one pass over the arrays, not
        // for a new schedule.  (Comparing array identity here would miss in-place edits of the arrays.)
        nativeSetRatings(handle, u, i, r);
        if (!initialised) {
            nativeInitFactors(handle, seed); // java.util.Random(seed).nextFloat()/sqrt(k), P then Q
            initialised = true;
        }
        double[] rmse = new double[epochs];
        nativeTrain(handle, epochs, rmse);
        return rmse;
    }

    public float predict(int u, int i) {
        return predict(new int[] {u}, new int[] {i})[0];
    }

    public float[] predict(int[] u, int[] i) {
        if (u.length != i.length) throw new IllegalArgumentException("length mismatch");
        float[] out = new float[u.length];
        nativePredict(handle, u, i, out);
        return out;
    }

    /** The topN best items of each user, best first (ties: smaller item index); scores as predict() gives them. */
    public int[][] recommend(int[] users, int topN) {
        int[] items = new int[users.length * topN];
        float[] scores = new float[users.length * topN];
        nativeRecommend(handle, users, topN, items, scores);
        int[][] out = new int[users.length][];
        for (int a = 0; a < users.length; a++) out[a] = java.util.Arrays.copyOfRange(items, a * topN, (a + 1) * topN);
        return out;
    }

    /**
     * The topN best of each row's candidates only ("the best 10 of these 500"), never item exclI[x] for user exclU[x].
     * candPtr == null: candItems is one list for every row; otherwise row a of users (the place in the array, not the
     * user: one user asked twice may carry two lists) owns candItems[candPtr[a] .. candPtr[a + 1]), candPtr having
     * users.length + 1 entries from 0 to candItems.length.  A list may be unsorted, repeat items (they count once) and
     * be empty.  Order and scores are recommend's; a row with fewer than topN eligible candidates gets -1 in the places left.
     */
    public int[][] recommendAmong(int[] users, int topN, long[] candPtr, int[] candItems, int[] exclU, int[] exclI) {
        if (exclU.length != exclI.length || (candPtr != null && candPtr.length != users.length + 1))
            throw new IllegalArgumentException("length mismatch");
        int[] items = new int[users.length * topN];
        float[] scores = new float[users.length * topN];
        nativeRecommendAmong(handle, users, topN, candPtr, candItems, exclU, exclI, items, scores);
        int[][] out = new int[users.length][];
        for (int a = 0; a < users.length; a++) out[a] = java.util.Arrays.copyOfRange(items, a * topN, (a + 1) * topN);
        return out;
    }

    /**
     * The seen-item index: what each user has already seen, built once on the device and kept there, so that the
     * ...Unseen calls serve "items this user has not seen" without the pair list.  setSeen: the index becomes the
     * distinct pairs (u[x], i[x]).
     */
    public void setSeen(int[] u, int[] i) {
        if (u.length != i.length) throw new IllegalArgumentException("length mismatch");
        nativeSeenUpdate(handle, 0, u, i);
    }

    /** The union of the index and the pairs: a merge on the device, the index is not sorted again. */
    public void markSeen(int[] u, int[] i) {
        if (u.length != i.length) throw new IllegalArgumentException("length mismatch");
        nativeSeenUpdate(handle, 1, u, i);
    }

    /** Drops the index and frees its device memory. */
    public void clearSeen() {
        nativeSeenUpdate(handle, 2, null, null);
    }

    /** Distinct pairs in the index; -1 when the model has none. */
    public long seenSize() {
        return nativeSeenSize(handle);
    }

    /** The seen items of the requested users, ascending within a user: list a belongs to users[a]. */
    public int[][] seen(int[] users) {
        int[] rowPtr = new int[users.length + 1];
        nativeGetSeen(handle, users, rowPtr, null);
        int[] items = new int[rowPtr[users.length]];
        if (items.length > 0) nativeGetSeen(handle, users, rowPtr, items);
        int[][] out = new int[users.length][];
        for (int a = 0; a < users.length; a++) out[a] = java.util.Arrays.copyOfRange(items, rowPtr[a], rowPtr[a + 1]);
        return out;
    }

    /** recommend(users, topN, exclU, exclI) with the pairs of the seen-item index, read on the device where they lie. */
    public int[][] recommendUnseen(int[] users, int topN) {
        return recommendUnseenAmong(users, topN, null, null);
    }

    /** recommendAmong with the pairs of the seen-item index; candItems == null: every item (recommendUnseen). */
    public int[][] recommendUnseenAmong(int[] users, int topN, long[] candPtr, int[] candItems) {
        if (candPtr != null && (candItems == null || candPtr.length != users.length + 1))
            throw new IllegalArgumentException("length mismatch");
        int[] items = new int[users.length * topN];
        float[] scores = new float[users.length * topN];
        nativeRecommendUnseen(handle, users, topN, candPtr, candItems, items, scores);
        int[][] out = new int[users.length][];
        for (int a = 0; a < users.length; a++) out[a] = java.util.Arrays.copyOfRange(items, a * topN, (a + 1) * topN);
        return out;
    }

    /** rankItems(u, i, exclU, exclI) with the pairs of the seen-item index. */
    public int[] rankItemsUnseen(int[] u, int[] i) {
        if (u.length != i.length) throw new IllegalArgumentException("length mismatch");
        int[] ranks = new int[u.length];
        nativeRankUnseen(handle, u, i, 0, null, ranks);
        return ranks;
    }

    /**
     * evaluateRanking with the pairs of the seen-item index: {nPairs, nUsers, hitRate, precision, recall, ndcg, mrr},
     * and the ranks into ranks (u.length entries; may be null).
     */
    public double[] evaluateRankingUnseen(int[] u, int[] i, int topN, int[] ranks) {
        if (u.length != i.length) throw new IllegalArgumentException("length mismatch");
        double[] metrics = new double[7];
        nativeRankUnseen(handle, u, i, topN, metrics, ranks != null ? ranks : new int[u.length]);
        return metrics;
    }

    /**
     * As recommend(users, topN), but never item exclI[x] for user exclU[x] (typically the arrays the model was trained
     * on, so that only unrated items come back).  A user with fewer than topN eligible items gets -1 in the places left.
     */
    public int[][] recommend(int[] users, int topN, int[] exclU, int[] exclI) {
        if (exclU.length != exclI.length) throw new IllegalArgumentException("length mismatch");
        int[] items = new int[users.length * topN];
        float[] scores = new float[users.length * topN];
        nativeRecommendExcluding(handle, users, topN, exclU, exclI, items, scores);
        int[][] out = new int[users.length][];
        for (int a = 0; a < users.length; a++) out[a] = java.util.Arrays.copyOfRange(items, a * topN, (a + 1) * topN);
        return out;
    }

    /**
     * Rows (nNew x k, row-major) for users that are not in the model: new user x owns ratings rowPtr[x] .. rowPtr[x + 1]
     * of items / ratings, and epochs passes of the per-rating SGD step run over them against the item factors, which
     * stay fixed.  init (nNew x k) gives the start rows; null: seeded rows, as a model of nNew users would start.
     * The model is not modified.
     */
    public float[] foldIn(long[] rowPtr, int[] items, float[] ratings, int epochs, float[] init, long seed) {
        if (rowPtr.length < 1 || items.length != ratings.length || items.length != rowPtr[rowPtr.length - 1])
            throw new IllegalArgumentException("length mismatch");
        int nNew = rowPtr.length - 1;
        if (init != null && init.length != nNew * k) throw new IllegalArgumentException("init must be nNew x k");
        float[] rows = new float[nNew * k];
        nativeFoldIn(handle, rowPtr, items, ratings, epochs, init, seed, rows);
        return rows;
    }

    /**
     * foldIn for items that are not in the model: new item x owns ratings rowPtr[x] .. rowPtr[x + 1] of users / ratings,
     * and the step runs against the user factors, which stay fixed.  The model is not modified; addItems(rows) puts the
     * rows into it.
     */
    public float[] foldInItems(long[] rowPtr, int[] users, float[] ratings, int epochs, float[] init, long seed) {
        if (rowPtr.length < 1 || users.length != ratings.length || users.length != rowPtr[rowPtr.length - 1])
            throw new IllegalArgumentException("length mismatch");
        int nNew = rowPtr.length - 1;
        if (init != null && init.length != nNew * k) throw new IllegalArgumentException("init must be nNew x k");
        float[] rows = new float[nNew * k];
        nativeFoldInItems(handle, rowPtr, users, ratings, epochs, init, seed, rows);
        return rows;
    }

    /**
     * Appends users to the live model and returns the index of the first: rows (n x k, row-major; for instance what
     * foldIn returned).  Nothing is rebuilt: the stored ratings, their schedules, the held-out set and the old rows stay
     * as they are, and with the factors on the device no old row leaves it.
     */
    public int addUsers(float[] rows) {
        if (rows.length % k != 0) throw new IllegalArgumentException("rows must be n x k");
        int first = nativeAppend(handle, SIDE_USERS, rows, rows.length / k, 0);
        users += rows.length / k;
        return first;
    }

    /** n seeded rows: foldIn's default start rows for this seed. */
    public int addUsers(int n, long seed) {
        int first = nativeAppend(handle, SIDE_USERS, null, n, seed);
        users += n;
        return first;
    }

    /** addUsers for items; rows: for instance what foldInItems returned. */
    public int addItems(float[] rows) {
        if (rows.length % k != 0) throw new IllegalArgumentException("rows must be n x k");
        int first = nativeAppend(handle, SIDE_ITEMS, rows, rows.length / k, 0);
        items += rows.length / k;
        return first;
    }

    public int addItems(int n, long seed) {
        int first = nativeAppend(handle, SIDE_ITEMS, null, n, seed);
        items += n;
        return first;
    }

    /**
     * Room for that many users / items in all (0: leave that side alone): appends up to there write in place, P and Q
     * keep their addresses and the cached training graphs stay valid.  Never shrinks.
     */
    public void reserve(int users, int items) {
        nativeReserve(handle, users, items);
    }

    /** {users, items} the model has room for without reallocating; the counts where nothing was reserved. */
    public int[] capacity() {
        int[] out = new int[2];
        nativeCapacity(handle, out);
        return out;
    }

    /**
     * recommend(users, topN, exclU, exclI) for rows (n x k) that are not in the model, such as foldIn's: row j plays
     * user j, and exclRow indexes rows.
     */
    public int[][] recommendRows(float[] rows, int topN, int[] exclRow, int[] exclItem) {
        if (exclRow.length != exclItem.length || rows.length % k != 0) throw new IllegalArgumentException("length mismatch");
        int n = rows.length / k;
        int[] items = new int[n * topN];
        float[] scores = new float[n * topN];
        nativeRecommendRows(handle, rows, topN, exclRow, exclItem, items, scores);
        int[][] out = new int[n][];
        for (int a = 0; a < n; a++) out[a] = java.util.Arrays.copyOfRange(items, a * topN, (a + 1) * topN);
        return out;
    }

    /** The two sides of the model for similarRows and rowInvNorms: rows of P, rows of Q. */
    public static final int SIDE_USERS = 0, SIDE_ITEMS = 1;

    private static int[][] rowsOf(int[] flat, int n, int topN) {
        int[][] out = new int[n][];
        for (int a = 0; a < n; a++) out[a] = java.util.Arrays.copyOfRange(flat, a * topN, (a + 1) * topN);
        return out;
    }

    /**
     * For each query item the topN other items whose rows of Q have the largest cosine with its row, best first (ties:
     * smaller index).  The query itself is never returned; with topN == items the last place of each row is -1.
     */
    public int[][] similarItems(int[] items, int topN) {
        int[] index = new int[items.length * topN];
        nativeSimilar(handle, SIDE_ITEMS, items, topN, index, new float[items.length * topN]);
        return rowsOf(index, items.length, topN);
    }

    /** similarItems among users: rows of P against P. */
    public int[][] similarUsers(int[] users, int topN) {
        int[] index = new int[users.length * topN];
        nativeSimilar(handle, SIDE_USERS, users, topN, index, new float[users.length * topN]);
        return rowsOf(index, users.length, topN);
    }

    /**
     * The neighbours of query vectors of the caller's (n x k: a folded-in user, a cold item's vector) among the rows of
     * Q (SIDE_ITEMS) or P (SIDE_USERS).  Nothing is excluded.
     */
    public int[][] similarRows(float[] rows, int topN, int side) {
        if (rows.length % k != 0) throw new IllegalArgumentException("length mismatch");
        int n = rows.length / k;
        int[] index = new int[n * topN];
        nativeSimilarRows(handle, side, rows, topN, index, new float[n * topN]);
        return rowsOf(index, n, topN);
    }

    /** 1 / sqrt(dot(row, row)) of every row of P (SIDE_USERS) or Q (SIDE_ITEMS), 0 for a zero row. */
    public float[] rowInvNorms(int side) {
        if (side != SIDE_USERS && side != SIDE_ITEMS) throw new IllegalArgumentException("side");
        float[] out = new float[side == SIDE_ITEMS ? items : users];
        nativeRowInvNorms(handle, side, out);
        return out;
    }

    /**
     * For each held-out pair (u[x], i[x]) the number of items that come before i[x] in u[x]'s recommendation order
     * (0: it would be recommended first), the pairs (exclU[x], exclI[x]) not competing -- the index of i[x] in the row
     * recommend(u[x], items, exclU, exclI) returns.  The held-out item itself is ranked even when a pair excludes it.
     */
    public int[] rankItems(int[] u, int[] i, int[] exclU, int[] exclI) {
        if (u.length != i.length || exclU.length != exclI.length) throw new IllegalArgumentException("length mismatch");
        int[] ranks = new int[u.length];
        nativeRankItems(handle, u, i, exclU, exclI, ranks);
        return ranks;
    }

    /** rankItems for rows (n x k) that are not in the model, such as foldIn's: row and exclRow index rows. */
    public int[] rankItemsRows(float[] rows, int[] row, int[] i, int[] exclRow, int[] exclItem) {
        if (row.length != i.length || exclRow.length != exclItem.length || rows.length % k != 0)
            throw new IllegalArgumentException("length mismatch");
        int[] ranks = new int[row.length];
        nativeRankItemsRows(handle, rows, row, i, exclRow, exclItem, ranks);
        return ranks;
    }

    /** What evaluateRanking returns: means over the users that have a held-out pair, and the rank of every pair. */
    public static final class RankingMetrics {
        public long nPairs, nUsers;
        public double hitRate, precision, recall, ndcg, mrr;
        public int[] ranks;
    }

    /**
     * rankItems(u, i, exclU, exclI) and the top-N metrics of those ranks at cut-off topN: hit rate, precision, recall
     * and NDCG at topN, and MRR.  The held-out pairs must be distinct for the figures to mean anything.
     */
    public RankingMetrics evaluateRanking(int[] u, int[] i, int topN, int[] exclU, int[] exclI) {
        if (u.length != i.length || exclU.length != exclI.length) throw new IllegalArgumentException("length mismatch");
        RankingMetrics m = new RankingMetrics();
        m.ranks = new int[u.length];
        double[] v = new double[7];
        nativeEvaluateRanking(handle, u, i, topN, exclU, exclI, v, m.ranks);
        m.nPairs = (long) v[0];
        m.nUsers = (long) v[1];
        m.hitRate = v[2];
        m.precision = v[3];
        m.recall = v[4];
        m.ndcg = v[5];
        m.mrr = v[6];
        return m;
    }

    public double rmse() {
        return nativeRmse(handle);
    }

    /**
     * Another learning rate and lambda for the live model (mfsgd_set_hyper): the schedules are re-baked in place,
     * nothing is rebuilt and the factors stay where they are.
     */
    public void setHyper(float lr, float lambda) {
        nativeSetHyper(handle, lr, lambda);
    }

    /** {lr, lambda} the model holds now. */
    public float[] hyper() {
        float[] out = new float[2];
        nativeGetHyper(handle, out);
        return out;
    }

    /**
     * One epoch per entry of {@code lr} over the ratings of the last train() call, epoch e at lr[e] and lambda[e]
     * ({@code lambda} null: the current one throughout); returns the RMSE after each epoch.  The model keeps the last
     * epoch's values.
     */
    public double[] trainSchedule(float[] lr, float[] lambda) {
        if (lambda != null && lambda.length != lr.length) throw new IllegalArgumentException("length mismatch");
        double[] rmse = new double[lr.length];
        nativeTrainSchedule(handle, lr, lambda, rmse);
        return rmse;
    }

    /**
     * {@code epochs} passes under the bold driver: after an epoch that lowered the RMSE the rate grows by {@code up},
     * otherwise it shrinks by {@code down}.  {@code lrUsed[e]} receives the rate of epoch e; returns the RMSE after
     * each epoch.  The model keeps the rate the next epoch would use.
     */
    public double[] trainBoldDriver(int epochs, float up, float down, float[] lrUsed) {
        if (lrUsed.length < epochs) throw new IllegalArgumentException("lrUsed shorter than epochs");
        double[] rmse = new double[epochs];
        nativeTrainBoldDriver(handle, epochs, up, down, lrUsed, rmse);
        return rmse;
    }

    /**
     * Applies fresh ratings of users and items the model already has, in the order given (mfsgd_apply_ratings): bit for
     * bit the sequential per-rating SGD loop at the current lr / lambda.  Returns each rating's error just before its
     * own update ("test, then train").  The ratings train() stored, their schedules and the held-out set are not
     * touched, and none is needed: a model that was only loaded can be updated.
     */
    public float[] partialFit(int[] u, int[] i, float[] r) {
        if (u.length != i.length || u.length != r.length) throw new IllegalArgumentException("length mismatch");
        float[] err = new float[u.length];
        nativeApplyRatings(handle, u, i, r, err);
        return err;
    }

    /**
     * The held-out set of the model (mfsgd_set_validation): copied, kept on the device from the first call that
     * measures it; empty arrays clear it.  Needs no GPU; survives train(), setHyper() and loadFactors().
     */
    public void setValidation(int[] u, int[] i, float[] r) {
        if (u.length != i.length || u.length != r.length) throw new IllegalArgumentException("length mismatch");
        nativeSetValidation(handle, u, i, r);
    }

    public long validationSize() {
        return nativeValidationSize(handle);
    }

    /** RMSE of the held-out set under the current factors; 0.0 for an empty set. */
    public double validationRmse() {
        double[] out = new double[2];
        nativeValidationRmse(handle, out);
        return out[0];
    }

    /** RMSE of the given pairs under the current factors (mfsgd_rmse_pairs): nothing is kept. */
    public double rmseOn(int[] u, int[] i, float[] r) {
        if (u.length != i.length || u.length != r.length) throw new IllegalArgumentException("length mismatch");
        double[] out = new double[2];
        nativeRmsePairs(handle, u, i, r, out);
        return out[0];
    }

    /** What trainEarlyStopping() did: the curves hold epochsRun entries ({@code trainRmse} null unless asked for). */
    public static final class EarlyStopping {
        public final double[] valRmse, trainRmse;
        public final int epochsRun, bestEpoch;

        EarlyStopping(double[] valRmse, double[] trainRmse, int epochsRun, int bestEpoch) {
            this.valRmse = valRmse;
            this.trainRmse = trainRmse;
            this.epochsRun = epochsRun;
            this.bestEpoch = bestEpoch;
        }
    }

    /**
     * Trains until the held-out RMSE has not improved by more than {@code minDelta} for {@code patience} epochs in a
     * row, at most {@code maxEpochs} epochs (mfsgd_train_early_stop states the rule); with {@code restoreBest} the model
     * ends with the factors of the best epoch.  {@code lr} / {@code lambda}: per-epoch values as in trainSchedule(),
     * maxEpochs entries each, or null for the current value throughout.
     */
    public EarlyStopping trainEarlyStopping(int maxEpochs, int patience, double minDelta, boolean restoreBest, float[] lr,
                                            float[] lambda, boolean trainRmse) {
        if (maxEpochs < 0) throw new IllegalArgumentException("negative maxEpochs");
        if ((lr != null && lr.length != maxEpochs) || (lambda != null && lambda.length != maxEpochs))
            throw new IllegalArgumentException("length mismatch");
        double[] val = new double[maxEpochs];
        double[] trn = trainRmse ? new double[maxEpochs] : null;
        int[] out = new int[2];
        nativeTrainEarlyStop(handle, maxEpochs, patience, minDelta, restoreBest ? 1 : 0, lr, lambda, val, trn, out);
        return new EarlyStopping(java.util.Arrays.copyOf(val, out[0]), trn == null ? null : java.util.Arrays.copyOf(trn, out[0]),
                                 out[0], out[1]);
    }

    /** P (users x k) and Q (items x k), row-major. */
    public float[][] factors() {
        float[] p = new float[users * k], q = new float[items * k];
        nativeGetFactors(handle, p, q);
        return new float[][] {p, q};
    }

    public void setFactors(float[] p, float[] q) {
        if (p.length != users * k || q.length != items * k) throw new IllegalArgumentException("shape mismatch");
        nativeSetFactors(handle, p, q);
        initialised = true;
    }

    // ---- DSGD over the GPUs of one node (include/mfsgd.h, "DSGD driver"; INTEGRATION.md section 5) -------------

    /** 128 bytes naming a new ring; rank 0 calls it and hands the bytes to every rank (any transport the host has). */
    public static byte[] distributedId() {
        return nativeDsgdUniqueId();
    }

    /**
     * The global partitioner: {userBegin[nParts + 1], itemPart[items]} from the two degree arrays of ONE global rating
     * set -- users in contiguous ranges balanced by rating count (rank g keeps users [userBegin[g], userBegin[g+1])),
     * items in partitions balanced by rating count with the chain-critical items packed together.  A pure function:
     * every rank computes the same plan.
     */
    public static int[][] plan(long[] degUser, long[] degItem, int nParts) {
        int[] userBegin = new int[nParts + 1], itemPart = new int[degItem.length];
        nativeDsgdPlan(degUser, degItem, nParts, userBegin, itemPart);
        return new int[][] {userBegin, itemPart};
    }

    /**
     * This rank's share of {@code epochs} DSGD epochs: {@code u} are LOCAL user indices (global index - userOffset),
     * {@code i} global item indices; {@code itemPart} (nullable: i % nParts) is plan()'s item map; the factors are seeded
     * as the single-device run over usersTotal x items would seed them.  Collective: every rank calls it with the same
     * {@code id}, world and epochs.  Returns the GLOBAL RMSE after each epoch.  The first call builds the schedules and
     * joins the ring (ncclCommInitRank); later calls on the same ratings only train.
     */
    public double[] trainDistributed(int[] u, int[] i, float[] r, int epochs, int rank, int world, byte[] id, int[] itemPart,
                                     long userOffset, long usersTotal) {
        if (nParts < 2) throw new IllegalStateException("created without item partitions");
        if (u.length != i.length || u.length != r.length) throw new IllegalArgumentException("length mismatch");
        if (id == null || id.length != 128) throw new IllegalArgumentException("id must be the 128 bytes of distributedId()");
        if (ring == 0) {
            if (itemPart != null) nativeSetItemPartition(handle, itemPart);
            nativeSetRatings(handle, u, i, r);
            nativeInitPOffset(handle, seed, userOffset); // P row u at stream position (userOffset + u) * k
            ring = nativeDsgdCreate(handle, rank, world, id);
            slots = nParts / world;
            nativeDsgdInitQ(ring, seed, usersTotal);     // Q row i at stream position (usersTotal + i) * k
            initialised = true;
        }
        double[] rmse = new double[epochs];
        nativeDsgdTrain(ring, epochs, rmse);
        return rmse;
    }

    /** Global RMSE with the current factors (collective). */
    public double rmseDistributed() {
        return nativeDsgdRmse(ring);
    }

    /** This rank's P rows (users x k, row-major). */
    public float[] userFactors() {
        float[] p = new float[users * k];
        nativeGetUserFactors(handle, p);
        return p;
    }

    /**
     * The Q blocks this rank holds between epochs: for slot j, {@code partOut[j]} receives the partition id and the
     * returned array its rows x k block (rows in ascending item id within the partition).
     */
    public float[][] itemBlocks(int[] partOut) {
        float[][] out = new float[slots][];
        int[] partRows = new int[2];
        for (int j = 0; j < slots; j++) {
            nativeDsgdGetQ(ring, j, partRows, null);
            out[j] = new float[partRows[1] * k];
            nativeDsgdGetQ(ring, j, partRows, out[j]);
            if (partOut != null) partOut[j] = partRows[0];
        }
        return out;
    }

    @Override
    public void close() {
        if (ring != 0) {
            nativeDsgdDestroy(ring);
            ring = 0;
        }
        if (handle != 0) {
            nativeDestroy(handle);
            handle = 0;
        }
    }

    // Every native throws RuntimeException(mfsgd_last_error) on a non-zero status.
    private static native long nativeCreate(int users, int items, int k, float lr, float lambda, int device, int nParts);
    private static native void nativeDestroy(long h);
    private static native void nativeSetRatings(long h, int[] u, int[] i, float[] r);
    private static native void nativeInitFactors(long h, long seed);
    private static native void nativeSetFactors(long h, float[] p, float[] q);
    private static native void nativeGetFactors(long h, float[] p, float[] q);
    private static native void nativeTrain(long h, int epochs, double[] rmsePerEpoch);
    private static native double nativeRmse(long h);
    private static native void nativeSetHyper(long h, float lr, float lambda);
    private static native void nativeGetHyper(long h, float[] lrLambda);
    private static native void nativeTrainSchedule(long h, float[] lr, float[] lambda, double[] rmsePerEpoch);
    private static native void nativeTrainBoldDriver(long h, int epochs, float up, float down, float[] lrUsed,
                                                     double[] rmsePerEpoch);
    private static native void nativeSetValidation(long h, int[] u, int[] i, float[] r);
    private static native long nativeValidationSize(long h);
    private static native void nativeValidationRmse(long h, double[] rmseSse);
    private static native void nativeRmsePairs(long h, int[] u, int[] i, float[] r, double[] rmseSse);
    private static native void nativeTrainEarlyStop(long h, int maxEpochs, int patience, double minDelta, int restoreBest,
                                                    float[] lr, float[] lambda, double[] valRmse, double[] trainRmse,
                                                    int[] epochsRunBestEpoch);
    private static native void nativeApplyRatings(long h, int[] u, int[] i, float[] r, float[] err);
    private static native void nativePredict(long h, int[] u, int[] i, float[] out);
    private static native void nativeRecommend(long h, int[] users, int topN, int[] items, float[] scores);
    private static native void nativeRecommendExcluding(long h, int[] users, int topN, int[] exclU, int[] exclI, int[] items,
                                                        float[] scores);
    private static native void nativeRecommendAmong(long h, int[] users, int topN, long[] candPtr, int[] candItems, int[] exclU,
                                                    int[] exclI, int[] items, float[] scores);
    private static native void nativeSeenUpdate(long h, int op, int[] u, int[] i);
    private static native long nativeSeenSize(long h);
    private static native void nativeGetSeen(long h, int[] users, int[] rowPtr, int[] items);
    private static native void nativeRecommendUnseen(long h, int[] users, int topN, long[] candPtr, int[] candItems, int[] items,
                                                     float[] scores);
    private static native void nativeRankUnseen(long h, int[] u, int[] i, int topN, double[] metrics7, int[] ranks);
    private static native void nativeFoldIn(long h, long[] rowPtr, int[] items, float[] ratings, int epochs, float[] init,
                                            long seed, float[] rows);
    private static native void nativeFoldInItems(long h, long[] rowPtr, int[] users, float[] ratings, int epochs, float[] init,
                                                 long seed, float[] rows);
    private static native int nativeAppend(long h, int side, float[] rows, int n, long seed);
    private static native void nativeReserve(long h, int users, int items);
    private static native void nativeCapacity(long h, int[] usersItems);
    private static native void nativeSimilar(long h, int side, int[] queries, int topN, int[] index, float[] scores);
    private static native void nativeSimilarRows(long h, int side, float[] rows, int topN, int[] index, float[] scores);
    private static native void nativeRowInvNorms(long h, int side, float[] out);
    private static native void nativeRankItems(long h, int[] u, int[] i, int[] exclU, int[] exclI, int[] ranks);
    private static native void nativeRankItemsRows(long h, float[] rows, int[] row, int[] i, int[] exclRow, int[] exclItem,
                                                   int[] ranks);
    private static native void nativeEvaluateRanking(long h, int[] u, int[] i, int topN, int[] exclU, int[] exclI,
                                                     double[] metrics7, int[] ranks);
    private static native void nativeRecommendRows(long h, float[] rows, int topN, int[] exclRow, int[] exclItem, int[] items,
                                                   float[] scores);
    // DSGD (mfsgd_dsgd_*, mfsgd_set_item_partition, mfsgd_init_p_offset)
    private static native byte[] nativeDsgdUniqueId();
    private static native void nativeDsgdPlan(long[] degUser, long[] degItem, int nParts, int[] userBegin, int[] itemPart);
    private static native void nativeSetItemPartition(long h, int[] itemPart);
    private static native void nativeInitPOffset(long h, long seed, long userOffset);
    private static native void nativeGetUserFactors(long h, float[] p);
    private static native long nativeDsgdCreate(long h, int rank, int world, byte[] id);
    private static native void nativeDsgdDestroy(long d);
    private static native void nativeDsgdInitQ(long d, long seed, long usersTotal);
    private static native void nativeDsgdTrain(long d, int epochs, double[] rmsePerEpoch);
    private static native double nativeDsgdRmse(long d);
    private static native void nativeDsgdGetQ(long d, int slot, int[] partRows, float[] block);
}
