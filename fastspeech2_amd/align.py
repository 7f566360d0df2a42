"""Forced alignment on the GPU: a left-to-right monophone HMM trained with Baum-Welch on the corpus itself and decoded with Viterbi,
writing the `{preprocessed_path}/TextGrid/{speaker}/{basename}.TextGrid` files that `Preprocessor` reads (the reference has no
aligner: its README sends the user to a Montreal Forced Aligner 1.x binary).  HIP kernels in fp64 over ragged batches
(csrc/fs2_align.hip).  The specification below is what the kernels and the numpy oracle (tests/align_ref.py) implement.  It is a
textbook flat-start monophone system (Rabiner 1989; the first stage of every HMM aligner); nothing here has been measured against
MFA, and the defaults marked "a choice" are choices, not measurements.

Features.  m[c, t] is the log-mel spectrogram `audio.TacotronSTFT` gives with the config's STFT settings for the whole file (no trim),
clamped to [-1, 1] first; T = samples // hop + 1 frames.  In float64 from here on: x[t, c] = m[c, t] - mean_t m[c, t] for c < n_mel,
x[t, n_mel + c] = (x[min(t + 1, T - 1), c] - x[max(t - 1, 0), c]) / 2.  D = 2 n_mel (160).

Lexicon and graph (host).  `path.lexicon_path` holds `word <blanks> phone phone ...` lines; the first pronunciation of a word wins and
lookup is lower-cased (the reference's `read_lexicon`).  A .lab's first line loses its trailing punctuation and is split at blanks
and at `, ; . - ? !` (synthesize.py `preprocess_english`); what is left of each piece after stripping punctuation from both ends is
a word, empty pieces are dropped.  A word the lexicon does not know is the one-phone word `spn`.  Blocks, in order: optional `sil`,
the phones of word 0, optional `sp`, the phones of word 1, ..., optional `sil`.  Every block has S states (1..3, default 2, a
choice: at hop 256 / 22050 Hz the shortest phone is then 23 ms); state j = block * S + s has emission class phone_id * S + s.
Predecessors of state j: j (self), j - 1 (next) and, when j is the first state of block k >= 2 and block k - 1 is optional, the last
state of block k - 2 (skip).  A path starts in state 0 or, block 0 being optional, in state S; it ends in state J - 1 or, the last
block being optional, in state J - 1 - S.  All arcs cost 0; transitions are not trained (with `transitions` = 1 they are: the
"Transitions" paragraph).  Per utterance: int32 arrays `sid`, `skip`
(-1 where there is none) and `block` of length J, and `alt` = (S, J - 1 - S).  M = the states of the mandatory blocks; an utterance
with T < M has no path: it is reported and skipped.  J above `max_states()` (1024) is a ValueError.

Emissions.  One diagonal Gaussian per class: E[t, j] = -1/2 sum_d ((x_d - mu_d)^2 / var_d + log(2 pi var_d)), in the direct form,
summed over d in ascending order (the kernel multiplies by 1 / var_d).

Training.  Flat start: frame t of an utterance belongs to its mandatory state number (t M) // T (optional blocks get nothing); the
first statistics are those of that hard assignment.  From their total the global mean g and variance v of the features follow;
every class starts at (g, v), the variance floor is 1e-2 v, and the update below is applied.  Then `iters` passes (default 12, a
choice).  A pass computes, per utterance, in the log domain (lse(a, b, c) = m + log(e^(a-m) + e^(b-m) + e^(c-m)), m the maximum, -inf
if m is -inf):
  alpha[0, j] = E[0, j] for the start states, else -inf;  alpha[t, j] = E[t, j] + lse(alpha[t-1, j], alpha[t-1, j-1], alpha[t-1, skip j])
  loglik = lse over the end states of alpha[T-1, .], in index order
  beta[T-1, j] = 0 for the end states, else -inf;  beta[t, j] = lse over the successors k = j, j + 1, the state that skips from j, of
  E[t+1, k] + beta[t+1, k];  gamma[t, j] = exp(alpha[t, j] + beta[t, j] - loglik)
and per class c the sums over all (utterance, state of class c) of  n = sum_t gamma,  a_d = sum_t gamma x_d,  q_d = sum_t gamma x_d^2.
Update: a class with n >= 1 gets mu = a / n, var = max(q / n - mu^2, floor); one with n < 1 keeps its parameters.  A pass reports
sum of loglik / sum of T, computed with the parameters it started from.

Decoding.  Viterbi with the same arcs: delta[t, j] = E[t, j] + max over (self, next, skip), backpointer 0 / 1 / 2, the lowest code on
ties; among the end states the lower index wins ties.  Backtracking gives frames per block; a skipped optional block has 0 frames
and is not written.  Block boundaries are at f hop / sampling_rate seconds, f the cumulative frame count; the last one is xmax.

Mixtures (`mixtures` = M > 1; the default M = 1 is everything above, unchanged).  Every HMM recipe (HTK, Kaldi, MFA) grows its
flat-start monophones into Gaussian mixtures by splitting; a single Gaussian cannot hold a phone that is realised in more than one
way (speakers, allophones, stress), its variance inflates until neighbouring phones overlap.
  Model.  Class c has K_c active components, 1 <= K_c <= M, M in 1..`max_mixtures()` (8).  Tables w (C, M), mu (C, M, D), var (C, M, D),
  float64.  Components m >= K_c are inactive: w = 0, mu = 0, var = 1, never updated.
  Emission.  For component m of the class of state j:  N[t, j, m] = log w_m - 1/2 sum_d ((x_d - mu_d)^2 / var_d + log(2 pi var_d)), the
  sum over d of the form and order above, log 0 = -inf.  E[t, j] = mx + log(sum_m exp(N_m - mx)), mx = max_m N_m, the sum over
  ascending m (-inf when mx is).  Responsibilities r[t, j, m] = exp(N_m - E[t, j]); a component with w = 0 gets exactly 0.  With M = 1
  and w = 1 this is the E above bit for bit (log 1 = 0, exp 0 = 1, mx + log 1 = mx).
  Statistics.  Per utterance partials [J][M][1 + 2 D]: the sum over ascending t of gamma[t, j] r[t, j, m] [1, x, x^2].  The class sums are
  the reduction above with component m of class c as row class c M + m and the partial row of (utterance b, state j, component m)
  as row (b ld_j + j) M + m, listed utterances first, then states ascending.
  Update (host, numpy).  n_c = sum over the active m of n_cm, ascending.  n_c >= 1: w_cm = n_cm / n_c; else the weights are kept.  An
  active component with n_cm >= 1 gets mu = a / n, var = max(q / n - mu^2, floor); one with n_cm < 1 keeps mu and var.  The floor is
  the one above.
  Schedule.  The flat start and the `iters` passes with one component, exactly as above; then for k = 1 .. M - 1: split, then
  `mix_iters` passes (default 4, a choice).
  Split of class c at step k.  h = the active component of the largest weight, the lowest index on ties.  If K_c < k + 1 and the
  occupancy n_ch of h in the last pass is at least `min_split_occ` (default 40 frames, a choice), component K_c becomes active: both
  halves get the weight w_h / 2, mu_new = mu_h + 0.2 sqrt(var_h), mu_h becomes mu_h - 0.2 sqrt(var_h), the variance is copied.  A
  class that fails the condition keeps its components (a rare `sp` or `spn` may never split).
  `fit` returns the log-likelihood per frame of every pass of every stage, in order, and logs K_c per stage.  Decoding takes E from
  the mixture emission (no responsibilities); Viterbi and backtracking are unchanged.  Nothing of this has been measured against MFA.

LDA (`lda` = k > 0; the default k = 0 is everything above, unchanged).  In HTK, Kaldi and MFA (`lda_mllt`) the stage after the
monophones is a linear discriminant transform of spliced frames.  Neighbouring mel channels are strongly correlated (overlapping
filters, a smooth envelope) and a diagonal Gaussian counts that shared variation once per channel; the other aligners decorrelate
with a DCT and LDA, this one has had neither.
  Switches.  `lda` = k output dimensions; `splice` = c frames of context on either side, 0..4, default 3; `lda_iters` passes after
  the transform, default 4.  c = 3 and k = 40 are Kaldi's customary values: here a choice, not a measurement.
  Spliced vector.  x is the feature matrix above; its first n_mel columns are the mean-removed static features.
  y[t, (p + c) n_mel + m] = x[min(max(t + p, 0), T - 1), m] for p = -c..c, m < n_mel; D_s = n_mel (2 c + 1).  The deltas are not
  spliced, the context replaces them.  1 <= k <= D_s <= `max_splice_dim()` (720); anything else is a ValueError (FS2_EINVAL at the
  ABI) before any launch.
  Statistics.  One extra pass with the single-Gaussian model the `iters` passes ended with, gamma its posteriors.  Per class c:
  n_c = sum gamma, a_c = sum gamma y (the reduction above, on y).  Over all frames of all utterances: N the frame count, s = sum y,
  S = sum y y^T.  Every frame's posteriors sum to 1, so the class sums and the totals describe the same mass.
  Transform (host, numpy float64).  m = s / N;  S_T = S / N - m m^T;  mu_c = a_c / n_c for the classes with n_c >= 1;
  S_B = sum_c n_c (mu_c - m)(mu_c - m)^T / N over those classes;  S_W = S_T - S_B + eps I, eps = 1e-8 trace(S_T) / D_s;
  S_W = L L^T (Cholesky);  `eigh` of L^-1 S_B L^-T, the k largest eigenvalues in descending order, eigenvectors v;  P holds the rows
  v^T L^-1, each sign-flipped so that its entry of largest magnitude is positive (the lowest index on ties);  o = P m.
  z[t] = P y[t] - o; the within-class covariance of z is the identity.
  Schedule.  (1) The flat start and the `iters` passes in x, exactly as above.  (2) The statistics pass and the transform.  (3) With
  the same gamma, one set of class sums on z gives the first (mu, var) in z-space (Kaldi's single-pass retraining); the global mean
  g and variance v of z follow from their total, a class with n < 1 starts at (g, v).  (4) The variance floor becomes 1e-2 v.
  (5) `lda_iters` Baum-Welch passes on z.  (6) The mixture stages, if `mixtures` > 1, on z.  (7) Decoding takes its emissions from z.
  `fit` returns the log-likelihood per frame of every pass as before, the statistics pass listed once between the passes in x and
  those in z, and logs the k eigenvalues.
  Sums.  S is summed over the lower triangle's 64 x 64 tiles with the fp64 matrix instruction, per chunk of padded frames (at most
  32 chunks, their length a function of the batch shape alone), frames ascending; the chunks are added in ascending order, the
  total is added to the table and mirrored, batch after batch in a fixed order.  Nothing of this has been measured against MFA,
  which cannot be run here, and nothing of it has been timed.

fMLLR (`fmllr` = 1; the default 0 is everything above, unchanged).  The stage after LDA in HTK, Kaldi (`train_sat`) and MFA (`sat`) is
speaker adaptation: constrained MLLR (Gales 1998, "Maximum likelihood linear transformations for HMM-based speech recognition",
section 3) estimates one affine feature transform per speaker by maximum likelihood and retrains the model in the normalised
space, so that the Gaussians need not absorb vocal-tract and channel differences into their variances (the failure of the
mixtures paragraph, one level up).  For a corpus of one speaker the same estimate is a global maximum-likelihood linear
transform, the MLLT half of `lda_mllt`.
  Notation.  f[t] is the D-dimensional feature the Gaussian stages see (z after `lda`, else x), xi[t] = (f[t], 1) has D + 1 entries.
  Speaker s owns W_s = [A_s | b_s] (D, D + 1), at first [I | 0]; the adapted feature is fh[t] = W_s xi[t].  1 <= D <=
  `max_fmllr_dim()` (64), anything else is a ValueError (FS2_EINVAL) before any launch: a speaker's statistics are D (D + 1)(D + 2)
  doubles, 2.2 MB at D = 64 and 33 MB at D = 160, so with 80 mel channels `fmllr` needs `lda` = k <= 64.  `build` also refuses,
  before any work, a corpus whose speaker tables (speakers x D (D + 1)(D + 2) x 8 bytes) exceed `resident_bytes`.
  Frame weights.  With gamma the state posteriors under the current single-Gaussian table (mu, var), for frame t and dimension i:
  c[t, i] = sum_j gamma[t, j] / var[sid_j, i],  h[t, i] = sum_j gamma[t, j] mu[sid_j, i] / var[sid_j, i], both over j ascending.
  Statistics.  Per speaker s over all frames of all its utterances: beta_s = the frame count, G_s[i] = sum_t c[t, i] xi[t] xi[t]^T
  (D + 1, D + 1), k_s[i] = sum_t h[t, i] xi[t] (D + 1).  xi is always taken from the unadapted f; gamma, mu and var come from the
  current model evaluated on fh.
  Update (host, numpy, `fmllr_update`).  A speaker with beta_s < `fmllr_min_frames` (default 500, Kaldi's value; here a choice) keeps
  W_s.  Otherwise every G_s[i] is inverted once; if a `np.linalg.cholesky(G_s[i])` raises, the speaker keeps W_s and is reported.
  Then `fmllr_sweeps` sweeps (default 20, a choice) over the rows i = 0 .. D - 1 in order:  p = (column i of A^-1, 0), A^-1 from
  `np.linalg.inv` of the current A at every row;  a = p G^-1 p^T;  c = p G^-1 k^T;  alpha = the root of a alpha^2 + c alpha - beta = 0
  with the larger beta log|alpha a + c| - a alpha^2 / 2, the '+' root on a tie;  row i of W becomes (alpha p + k) G^-1.  This is
  Gales's row-by-row maximiser of beta log|det A| - 1/2 sum_i (w_i G_i w_i^T - 2 w_i k_i^T), which cannot decrease at any row step.
  Schedule.  Every stage up to and including the `lda_iters` passes (without `lda`: the `iters` passes) runs unchanged.  Then
  `fmllr_rounds` rounds (default 2, a choice), each: (a) a statistics pass: posteriors on fh, frame weights, accumulation; (b) the
  update; (c) fh recomputed; (d) `fmllr_iters` Baum-Welch passes on fh (default 2, a choice) with the variance floor of the stage
  before.  The mixture stages and decoding then run on fh with the transforms frozen; re-estimating the transforms under mixtures
  is out of scope.  From the first statistics pass on `fit` reports per pass (sum_u loglik_u + T_u log|det A_s(u)|) / n_frames, so
  the numbers stay comparable across the stage and the pass after an update does not report less than the statistics pass before
  it.  `fit` prints one line per round: speakers adapted, speakers kept (too few frames / not positive definite), the mean
  log|det A|.  `fit` and `align` take the speaker index of every utterance; with `fmllr` on, a missing list or an index that is
  negative or outside the speakers `fit` saw is a ValueError.
  Sums.  G_s[i] is summed over the lower triangle's 16 x 16 tiles with the fp64 matrix instruction, the frame its k index, c[t, i] xi[t]
  one operand and xi[t] the other.  A speaker's utterances are taken in batch-row order, frames ascending; its padded frames are cut
  into chunks (their length a function of the batch shape alone) whose partial sums are added in ascending chunk order, the total
  is added to the table and mirrored (G_s[i] is exactly symmetric), batch after batch in the fixed order.  Tables of speakers with
  no utterance in a batch are not touched by it.  Nothing of this has been measured against MFA, which cannot be run here, and
  nothing of it has been timed.

Triphones (`triphones` = L > 0 leaves; the default 0 is everything above, unchanged).  The stage between the monophones and the
LDA in HTK, Kaldi and MFA (`monophone -> triphone -> lda_mllt -> sat`): coarticulation makes the first state of a phone depend on
what precedes it and the last on what follows; a context-independent Gaussian absorbs that into its variance and mixtures can
only answer it blindly, while the context is known from the transcript.  The triphones are word-internal (HTK's classic system)
and tied by a likelihood decision tree (Young, Odell and Woodland 1994, "Tree-based state tying for high accuracy acoustic
modelling").
  Context (host, `triphone_contexts`).  A mandatory block of phone p in word w has the left context l = the phone of the previous
  block if that block belongs to word w, else the boundary symbol `#`; r likewise from the next block.  Context never crosses a word
  boundary, so it does not depend on whether an optional `sp` or `sil` is taken; the graph (`skip`, `block`, `alt`) is untouched, only
  `sid` changes.  `sil`, `sp` and `spn` are context-independent: l = r = `#`, they are never a context and are never split.  A logical
  state is (l, p, r, s); symbols are the phone ids and `#` = the number of phones.
  Placement (a choice).  After the last single-Gaussian stage (the `iters` passes in x, the passes in z after `lda`, the passes on
  the adapted features after `fmllr`) and before the mixtures: every earlier stage stays bit-identical and the tree is grown in
  the best feature space the run has.  f is the feature those stages see, D its dimension, floor their variance floor.
  Statistics pass.  Posteriors under the monophone table; partials with `fs2_align_stats`, reduced with `fs2_align_reduce` over an
  index whose classes are the items: the distinct logical states seen in the corpus, numbered in sorted (p, s, l, r) order.  The
  item sums (N_items, 1 + 2 D) stay on the device.  The pass is listed once in the history.  `build` refuses, before any work, a
  table that may exceed `resident_bytes` (at most R S (R + 1)^2 + 3 S rows for R real phones).
  Questions (host, numpy).  A question is (side, set of symbols); with n_sets sets, question q < n_sets asks whether l is in set q,
  question n_sets <= q < 2 n_sets whether r is in set q - n_sets.  By default the sets come from a bottom-up clustering of the real
  phones (the idea of Kaldi's `cluster-phones`): start from singletons; merge the pair of clusters with the smallest
  sum_s (L_s(A) + L_s(B) - L_s(A u B)), L as below on the monophone sums pooled from the item sums (items ascending), a cluster
  named by its lowest phone and ties going to the lowest pair; every singleton (ascending), every merged set (in merge order) except
  the full set, and `{#}` are the 2 P - 1 sets.  `questions` = a file replaces them: one set per line, `name phone phone ...`, `#` the
  boundary; an unknown phone is a ValueError.  At most `max_tree_sets()` (1024) sets, more is a ValueError (FS2_EINVAL).
  Likelihood.  L(n, a, q) = -n / 2 sum_d (log(2 pi v_d) + 1), v_d = max(q_d / n - (a_d / n)^2, floor_d), d ascending; 0 for n = 0.
  Tree.  One root per (p, s), node p S + s, holding that state's items; the roots of `sil`, `sp` and `spn` are leaves from the start.
  A split of a node by question q is eligible when both sides have n >= `tri_min_occ` (default 100 frames, HTK's RO value, here a
  choice; below 1 is a ValueError); its gain is (L(yes) + L(no)) - L(node); an ineligible split has gain -inf and no variance is
  formed for it.  A node's best split is the largest gain, the lowest q on ties; the node splits if that gain exceeds
  `tri_min_gain` (default 0, a choice).  The full tree is built level by level, all open nodes of a level in one launch
  (`tree_gains`); the children of a level are numbered in ascending parent order, yes before no.
  Budget.  The recorded splits are replayed on the host through a priority queue, the largest gain first, the lowest node number on
  ties, until L leaves exist or no split is left: a node's best gain does not depend on other nodes, so this is best-first
  splitting without one launch per split.  L below the number of roots (fixed leaves included) is a ValueError.  Leaves are
  numbered in ascending node order.
  Leaf table.  Each leaf gets (mu, var) by the update above on its pooled item sums (items ascending), starting from its root's
  monophone parameters: a leaf with n < 1 (a root whose phone never occurs) keeps them.
  Passes.  Graphs are rebuilt with `sid` = the leaf that the state's (p, s, l, r) reaches from its root; any triple reaches a leaf,
  seen in training or not, so `align` works on new utterances.  The number of classes becomes the leaf count; `tri_iters`
  Baum-Welch passes (default 4, a choice) with the floor unchanged, then the mixture stages on the leaves, decoding on the leaves.
  `fit` logs the number of items, questions and leaves and the total gain, and keeps the tree as arrays over the nodes: the question,
  the yes child, the no child, the leaf id, each -1 where there is none.
  Sums.  For a node's items the yes-sums and the no-sums of every question are both accumulated directly with the fp64 matrix
  instruction (a 0/1 matrix times the item table, the item its k index, ascending in steps of four); the order of every sum
  depends on the node's item count and D alone, and a question's arithmetic does not depend on where it sits in the table: two
  sets that part a node's items alike tie bit for bit and the lower index wins.  Nothing of this has been measured against MFA,
  which cannot be run here, nothing is known about its gain on real speech, and nothing of it has been timed.

Transitions (`transitions` = 1; the default 0 is everything above, unchanged: the same launches, the same numbers, the same bytes).
Every HMM recipe (HTK, Kaldi, MFA) re-estimates, together with the Gaussians, the state transition probabilities and the
probabilities of the optional silences; these are the arc posteriors xi of textbook Baum-Welch (Rabiner 1989).  Without them the
choice between taking and skipping an `sp` rests on the emissions of one or two frames, and a state's expected duration carries
no weight.  The graph topology, the emission stages and the flat start are untouched.
  Tables (host, numpy float64, attributes of `Aligner`).  loop (n_classes,): the self-loop probability of every emission class,
  tied exactly as the emissions are: per monophone state, per leaf after `triphones` (a leaf starts from its root's value); the
  mixture components of a class share one value.  opt (3,): the probability that an optional block is taken; kind 0 is an optional
  block at block index 0, kind 2 one at the last block index, kind 1 any other (`sp`).  All entries start at 0.5 (a choice); every
  probability is clipped to [TRANS_FLOOR, 1 - TRANS_FLOOR], TRANS_FLOOR = 0.01 (Kaldi's transition floor; here a choice), so every
  arc cost is finite.
  Arc costs (host, `arc_costs`), per utterance w (3, J) and edge (4,), kind(k) the kind of optional block k:
  w[0, j] = log loop[sid[j]] (self);  w[1, j], the arc j - 1 -> j, = log(1 - loop[sid[j - 1]]), plus log opt[kind(block[j])] when j is
  the first state of an optional block (w[1, 0] = 0, unused);  w[2, j], the arc skip[j] -> j, = log(1 - loop[sid[skip[j]]]) +
  log(1 - opt[kind(block[j] - 1)]), 0 where skip[j] < 0;  edge[0], start in state 0, = log opt[0] if block 0 is optional, else 0;
  edge[1], start in state alt[0], = log(1 - opt[0]);  edge[2], end in state J - 1, = log(1 - loop[sid[J - 1]]);  edge[3], end in
  state alt[1], = log(1 - loop[sid[alt[1]]]) + log(1 - opt[2]).  Leaving a state is a proper distribution: self, next, the skip
  that starts there and the end edge where there is one sum to 1.
  Recursions.  alpha[0, j] = edge + E[0, j] at the start states;  alpha[t, j] = E[t, j] + lse(alpha[t-1, j] + w[0, j], alpha[t-1, j-1] +
  w[1, j], alpha[t-1, skip j] + w[2, j]);  loglik = lse over the end states e of alpha[T-1, e] + edge(e), in index order;
  beta[T-1, e] = edge(e) at the end states, and the backward recursion adds the cost of every successor arc;  gamma as above.
  Viterbi takes the same costs inside its max with the tie rules unchanged (the lowest backpointer code, then the lower end
  index); backtracking is unchanged.
  Arc posteriors.  For a in (self, next, skip):  xi[j, a] = sum over t = 1 .. T - 1 of exp(alpha[t-1, pred_a(j)] + w[a, j] + E[t, j] +
  beta[t, j] - loglik), summed in descending t, the order in which the backward scan visits the frames (no floating-point
  atomics).  Two further columns hold the start mass gamma[0, j] and the end mass gamma[T - 1, j], so the host never slices gamma.
  xi[j].sum over the arcs + gamma[0, j] = sum_t gamma[t, j].
  Update (host, `trans_step`, beside `m_step`).  With n_c the class occupancy (column 0 of the class sums; under mixtures the sum
  over the active components, ascending) and s_c the class sum of xi[:, self]: a class with n_c >= 1 gets loop_c = clip(s_c / n_c),
  any other keeps its value.  This is the exact maximum-likelihood estimate: a frame's mass either loops or leaves, the last
  frame's through the end edge.  Per kind, `enter` and `skipped` are summed over the corpus: kind 1, xi[first state of the block,
  next] and xi[first state of the block after it, skip]; kind 0, gamma[0, 0] and gamma[0, alt[0]]; kind 2, xi[J - S, next] and
  gamma[T - 1, alt[1]].  opt_k = clip(enter / (enter + skipped)) when enter + skipped >= 1, else it is kept.  All corpus sums go
  through `fs2_align_reduce` with host-built lists (the class list of the statistics; the list of the optional blocks, utterances
  then blocks ascending), batch after batch in the fixed order: two runs are bit-identical.
  Schedule.  The flat start is unchanged.  Every Baum-Welch pass of every stage (`iters`, `lda_iters`, the passes of the fMLLR
  rounds, `tri_iters`, the mixture passes) runs under the current arc costs and updates loop and opt together with the Gaussians;
  the statistics-only passes (LDA, fMLLR, tree) take their posteriors under the current costs and update nothing; `align`
  decodes with the trained costs.  `fit`'s history keeps its meaning and now includes the arc terms (the fMLLR Jacobian is added
  as before); `fit` logs one line per stage with opt and the range of 1 / (1 - loop), the expected frames per state.  With every
  entry at 0.5 every path of an utterance carries the same arc total, (T + the number of its optional blocks) log 0.5, so the
  posteriors of the first pass equal the default run's: that is why 0.5 is a harmless start.
  Quality against MFA unmeasured (it cannot be run here); transition probabilities are known to matter less than emissions, the
  silence probabilities more; what either changes on real speech is unknown, and no timing measured yet.

Confidence (`scores` = a file; without it every launch, number and TextGrid byte is everything above, unchanged).  Viterbi always
returns some path: a .lab that does not match its audio (a word misread, skipped or added, a number expanded otherwise, a lexicon's
first pronunciation that is not the spoken one, an OOV word turned into `spn`) is aligned as confidently as a clean one.  The
scores below say per phone interval how well the model agrees with what the transcript claims; they are model-based and intrinsic.
  Feature.  f[t] is the feature the decoding model sees (x, z after `lda`, the adapted fh after `fmllr`), D its dimension, C =
  `n_classes` at decode time (monophone states, or leaves after `triphones`), M = `mixtures`.
  Class score.  F[t, c] is the acoustic log-likelihood of frame t under class c in the form of the "Emissions" and "Mixtures"
  paragraphs: the direct form, multiplied by 1 / var_d, d ascending; with M > 1 the log-sum over ascending m of log w_m + N_m; a
  component of weight 0 contributes -inf; with M = 1 the weight is 1.  No arc costs enter F.  The kernel takes 1 / var_d and, per
  component, log w - 1/2 sum_d log(2 pi var_d) (d ascending) once per call, and folds the components with a running maximum, so F
  agrees with `emit` / `emit_gmm` to rounding, not bit for bit.
  Path.  s[t] is the state of the Viterbi path at frame t, the path `align` decodes (under the arc costs when `transitions` = 1);
  p[t] = sid[s[t]] is its class.
  Per frame.  own[t] = F[t, p[t]];  best[t] = max_c F[t, c];  arg[t] = the lowest c that attains the maximum.  All three come from one
  kernel and one code path per class: own[t] <= best[t] holds exactly, and own[t] == best[t] bit for bit where arg[t] == p[t].  A
  class's arithmetic does not depend on its index or on where it sits in a tile: two classes with identical table rows tie bit for
  bit and the lower index wins (the property the tree paragraph demands of its questions).  The T x C matrix is never stored.
  Per block (a TextGrid phone interval) of n > 0 frames, sums over ascending t:  `loglik` = (1/n) sum own[t];  `gop` = (1/n) sum
  (own[t] - best[t]), always <= 0, and 0 when the aligned class wins every frame;  `match` = the share of the block's frames with
  class_phone[arg[t]] == the block's phone.  class_phone (C,): c // S for monophone states, the phone of the leaf's root for
  leaves (`Aligner.class_phone`).  `gop` is the goodness of pronunciation of Witt and Young (2000, "Phone-level pronunciation
  scoring and assessment for interactive language learning") with the free phone loop replaced by the frame-wise maximum over
  the classes: the usual approximation, and an approximation (the maximum is free to change class at every frame and pays no arc
  cost, so it is an upper bound of any phone loop's score).  A block of 0 frames has NaN and is not written.
  Per utterance.  `frames`;  `viterbi` = the Viterbi score / T (the third value `viterbi*` returns; it includes the arc costs when
  they are trained);  `gop` and `match` = the same means over the frames of all mandatory blocks (`scored_frames` of them): optional
  `sil` / `sp` are left out, `spn` is included and recognisable by its label;  `loglik` over all frames.
  fMLLR.  With `fmllr`, `loglik` and `viterbi` are in the adapted space without the Jacobian: they compare within a speaker.  `gop`
  and `match` are differences and shares, they compare across speakers.
  File.  One JSON object per written utterance and line: speaker, basename, the utterance numbers, and phones = [label, start_s,
  end_s, loglik, gop, match] per written interval, the TextGrid's own boundaries.  The block means are taken on the host (numpy) from
  the per-frame arrays; 28 bytes a frame come back from the device.
  What is claimed.  Nothing here is a threshold: no default cut-off is shipped, no TextGrid is dropped or changed, and which `gop`
  separates a wrong transcript from a right one on real speech is unmeasured.  On the synthetic corpus of the tests a substituted
  word scores below the untouched words of its utterance in all 8 fixed cases; that is all that is known.  The summary line prints
  the corpus mean and the 10 utterances of lowest `gop` for a person to look at.  Two runs (`triphones` against none, `mixtures`
  4 against 1) can be compared on how sharply they separate right from wrong transcripts; quality against MFA stays unmeasured.

Segmental scores (`seg_scores` = 1, needs `scores`; without it every launch, number, TextGrid byte and scores-file byte is everything
above, unchanged).  `gop` above replaces Witt and Young's denominator, the best phone hypothesis for the segment, by a maximum that
may change class at every frame and pays no arc cost: an upper bound that does not say which phone the model would rather have
heard.  This paragraph is the definition as published (Witt and Young 2000, eq. 3): log p(O_seg | p) minus max_q log p(O_seg | q)
over the number of frames, every q scored as a whole HMM over the same segment, and it names the winning q.
  Segment.  Block k of an utterance with n > 0 frames [a, a + n) on the decoded Viterbi path (`segment_table`); the blocks partition
  the frames.
  Candidates (`Aligner.candidates`).  P is the number of phones of the phone table (`sil`, `sp` and `spn` included), S the states
  per phone.  For every block k, phone q < P and state s < S the candidate class cand[k, q, s] is q S + s for monophone models and,
  after `triphones`, the leaf that (l_k, q, r_k, s) reaches from root q S + s.  l_k and r_k are the block's own transcript contexts
  as `triphone_contexts` gives them; l = r = `#` when the block's phone or q is one of the context-independent `sil` / `sp` / `spn`.
  Only the block's own states are substituted, its neighbours keep their transcript contexts: an approximation (a rival phone
  would also change the context of the phones beside it).
  Class score.  F[t, c] exactly as in the Confidence paragraph: the direct form, 1 / var_d and the per-component constant prepared
  once per call, d ascending, the mixture fold with a running maximum, a component of weight 0 contributing -inf.
  Segment score.  With c_s = cand[k, q, s]:  ws_s = log loop[c_s] and wn_s = log(1 - loop[c_s]) when `transitions` = 1, both 0
  otherwise.  v_0(a) = F[a, c_0] and v_s(a) = -inf for s > 0;  v_s(t) = F[t, c_s] + max(v_s(t-1) + ws_s, v_{s-1}(t-1) + wn_{s-1});
  V[k, q] = v_{S-1}(a + n - 1) + wn_{S-1}, -inf when n < S.  This is the block's own topology: no skip inside a block, every state
  occupied at least one frame.  The exit arc is included because it differs per candidate; the entry costs (`opt`) are the same
  for all candidates and are left out.
  Per written interval, p the interval's phone.  `rival` = the lowest q != p that attains max_{q != p} V[k, q];  `margin` = (V[k, p] -
  V[k, rival]) / n, positive when the transcript's phone wins;  `gop_seg` = min(margin, 0), Witt and Young's number, always <= 0.
  With P = 1 there is no rival: null, null and 0 are written.
  Per utterance.  `gop_seg` = the frame-weighted mean over the mandatory blocks, the frames `gop` uses.
  Relations.  V[k, p] >= the forced path's own score over the segment, sum own[t] plus its internal and exit arcs, and equal to it
  up to rounding unless the segment has a tie (the forced path is the best path through the block's states; its entry and the
  rest of the utterance do not depend on how the block's frames are shared out).  Without `transitions`: gop <= gop_seg <= 0 per
  block up to rounding, since sum best[t] bounds every V[k, q] from above and V[k, p] bounds the own sum from above.
  Kernel (csrc/fs2_align_seg.hip).  One workgroup per (utterance, block); F is computed for 16 frames x 64 candidate columns at a
  time with the statements of the frame-score kernel and one lane per candidate phone advances v over the frames, so a class's
  arithmetic does not depend on where it sits: two phones with identical table rows get bit-identical V and the lower one is the
  rival.  No floating-point atomics; every sum ascends in t and d: two runs are bit-identical.  A segment with frames <= 0, start <
  0 or start + frames > T, or a candidate row holding -1, is absent: its V row keeps the NaN of a fresh buffer.  A candidate class
  >= n_classes is a ValueError before the launch (the kernel scores such a column -inf without reading the table); P above
  `max_seg_phones()` (256), S outside 1..3 and M outside 1..8 are ValueErrors (FS2_EINVAL) before the launch.
  File.  Every phone entry becomes [label, start_s, end_s, loglik, gop, match, gop_seg, rival_label, margin] and the utterance object
  gains `gop_seg`; the summary appends the corpus mean `gop_seg` and the 20 most frequent (phone -> rival) pairs among the
  intervals with margin < 0, with their counts.
  What is claimed.  The published definition, pinned to a numpy restatement (tests/align_seg_ref.py).  No threshold.  Nothing has
  been measured on real speech, against MFA or against Kaldi's `compute-gop`, and no timing measured yet.

Model files (`save_model` / `model`; without them every launch, number and byte is everything above, unchanged).  `Aligner.save`
writes one .npz without pickled objects: the tables the decoding model uses (mu / var, or gw / gmu / gvar / ncomp; P / o; W; the
tree's arrays; loop / opt; floor), the constructor options, the phone table in id order, the feature settings the model was trained
under (sampling rate, filter / hop / win length, n_mel, fmin, fmax), with `fmllr` the speaker names in index order, the phone bigram
counts of the training corpus's decoded alignments (a sequence is the blocks with frames > 0, the realised `sil` / `sp` included;
fastspeech2_amd/recognize.py) and MODEL_VERSION.  `Aligner.load` rebuilds an `Aligner` whose `align` and `score` return the bits of
the original's.  `build(..., model=file)` trains nothing (the history is []) and aligns the corpus with the loaded model; it
refuses, with a ValueError naming the difference and before any audio is read, training options beside the file, a lexicon whose
phone table is not the model's, feature settings that are not the model's and, with `fmllr`, a speaker directory the model has no
transform for (estimating transforms for new speakers is not built).

Determinism.  No floating-point atomics.  Per utterance the sums go to partials [J][1 + 2 D], each summed in ascending t; the class
sums add those rows in the order of a host-built (class -> [(utterance, state)]) list, batch after batch in a fixed order; the
update runs on the host in numpy.  Every sum's order is a function of the batch shape (for the speaker statistics: and of the
batch's speaker list) only.  Two runs over one corpus write byte-identical TextGrids.
"""
import json
import os
import re
from concurrent.futures import ThreadPoolExecutor
from string import punctuation

import numpy as np
import torch

from . import _lib, ops, ragged

SIL, SP, SPN = "sil", "sp", "spn"
VAR_FLOOR = 1e-2
TRANS_FLOOR = 0.01
_SPLIT = re.compile(r"[,;.\-\?\!\s+]")


def _up(a, device):
    """A numpy array on the device."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _csr(classes, n, device, rows=None):
    """CSR (class -> the rows of that class, in their given order) of a class vector over n classes: (offs (n + 1,), items) int32
    on the device.  `rows` names the row of every entry (default: its position).  Never an empty item tensor: the lists bound
    what is read."""
    classes = np.asarray(classes, np.int64)
    order = np.argsort(classes, kind="stable")
    offs = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(classes, minlength=n), out=offs[1:])
    items = order if rows is None else np.asarray(rows, np.int64)[order]
    return _up(offs.astype(np.int32), device), _up((items if items.size else np.zeros(1)).astype(np.int32), device)


# ------------------------------------------------------------------------------------------------ lexicon, text, graph
def read_lexicon(path):
    lexicon = {}
    with open(path, encoding="utf-8") as f:
        for line in f:
            parts = line.split()
            if parts and parts[0].lower() not in lexicon:
                lexicon[parts[0].lower()] = parts[1:]
    return lexicon


def words_of(text):
    """The words of one .lab line: trailing punctuation dropped, split as `preprocess_english` splits, punctuation stripped."""
    pieces = (w.strip(punctuation) for w in _SPLIT.split(text.strip().rstrip(punctuation)))
    return [w for w in pieces if w]


def pronounce_oov(transcripts, lexicon, phone_ids, g2p):
    """Out-of-lexicon words through a trained grapheme-to-phoneme model (fastspeech2_amd/g2p.py): every word of `transcripts` (lists of
    words) that `lexicon` lacks is pronounced in ONE batched decode; a pronunciation is taken when the model has one and every phone
    of it is in `phone_ids`, else the word stays out (and becomes `spn`).  -> (lexicon with the taken words added, taken, left)."""
    oov = sorted({w.lower() for words in transcripts for w in words} - set(lexicon))
    if not oov:
        return lexicon, 0, 0
    said = {w: p for w, p in zip(oov, g2p.pronounce(oov)) if p and all(q in phone_ids for q in p)}
    return {**lexicon, **said}, len(said), len(oov) - len(said)


def phone_table(lexicon):
    """phone -> id over the lexicon's phones, sorted, then sil, sp, spn."""
    phones = sorted({p for ps in lexicon.values() for p in ps} - {SIL, SP, SPN})
    return {p: i for i, p in enumerate(phones + [SIL, SP, SPN])}


def utterance_graph(words, lexicon, phone_ids, states=2):
    """-> dict(sid, skip, block: int32 [J]; alt: (start, end) alternatives or -1; blocks: [(phone, word index or -1, optional)];
    mandatory: number of states every path visits)."""
    if not 1 <= states <= 3:
        raise ValueError(f"states must be 1..3, got {states}")
    if not words:
        raise ValueError("an utterance needs at least one word")
    blocks = [(SIL, -1, True)]
    for w, word in enumerate(words):
        if w:
            blocks.append((SP, -1, True))
        for p in lexicon.get(word.lower()) or [SPN]:
            blocks.append((p, w, False))
    blocks.append((SIL, -1, True))
    S, J = states, len(blocks) * states
    sid, skip, block = np.empty(J, np.int32), np.full(J, -1, np.int32), np.empty(J, np.int32)
    for k, (p, _, _) in enumerate(blocks):
        for s in range(S):
            sid[k * S + s] = phone_ids[p] * S + s
            block[k * S + s] = k
        if k >= 2 and blocks[k - 1][2]:
            skip[k * S] = (k - 1) * S - 1
    alt = (S if blocks[0][2] else -1, J - 1 - S if blocks[-1][2] else -1)
    return {"sid": sid, "skip": skip, "block": block, "alt": alt, "blocks": blocks,
            "mandatory": S * sum(1 for b in blocks if not b[2])}


def flat_assignment(graph, T):
    """Flat start: the state of every frame, frame t -> mandatory state number (t M) // T."""
    opt = np.array([b[2] for b in graph["blocks"]])
    mand = np.nonzero(~opt[graph["block"]])[0]
    return mand[(np.arange(T, dtype=np.int64) * len(mand)) // T]


def m_step(sums, mu, var, floor):
    """The update of the module docstring on class sums [C][1 + 2 D] -> (mu, var)."""
    D = mu.shape[1]
    n = sums[:, 0]
    ok = n >= 1.0
    nn = np.where(ok, n, 1.0)[:, None]
    m = sums[:, 1:1 + D] / nn
    v = np.maximum(sums[:, 1 + D:] / nn - m * m, floor[None, :])
    return np.where(ok[:, None], m, mu), np.where(ok[:, None], v, var)


def m_step_gmm(sums, w, mu, var, ncomp, floor):
    """The mixture update of the module docstring on class sums (C, M, 1 + 2 D) -> (w, mu, var); inactive components are left alone."""
    C, M, D = mu.shape
    sums = np.asarray(sums).reshape(C, M, 1 + 2 * D)
    active = np.arange(M)[None, :] < np.asarray(ncomp)[:, None]
    n = np.where(active, sums[:, :, 0], 0.0)
    n_c = np.zeros(C)
    for m in range(M):                                                     # ascending m, as specified
        n_c = n_c + n[:, m]
    keep_w = n_c < 1.0
    w_new = np.where(keep_w[:, None] | ~active, w, n / np.where(keep_w, 1.0, n_c)[:, None])
    ok = active & (n >= 1.0)
    nn = np.where(ok, n, 1.0)[:, :, None]
    m_new = sums[:, :, 1:1 + D] / nn
    v_new = np.maximum(sums[:, :, 1 + D:] / nn - m_new * m_new, floor[None, None, :])
    return w_new, np.where(ok[:, :, None], m_new, mu), np.where(ok[:, :, None], v_new, var)


def split_classes(w, mu, var, ncomp, occ, k, min_split_occ=40.0, step=0.2):
    """Split step k of the module docstring: occ (C, M) is the occupancy of every component in the last pass -> (w, mu, var, ncomp)."""
    w, mu, var, ncomp = w.copy(), mu.copy(), var.copy(), np.array(ncomp, dtype=np.int64)
    occ = np.asarray(occ).reshape(w.shape)
    for c in range(w.shape[0]):
        K = int(ncomp[c])
        h = int(np.argmax(w[c, :K]))                                       # the first of the largest
        if K < k + 1 and K < w.shape[1] and occ[c, h] >= min_split_occ:
            d = step * np.sqrt(var[c, h])
            w[c, h] = w[c, K] = w[c, h] / 2.0
            mu[c, K], mu[c, h] = mu[c, h] + d, mu[c, h] - d
            var[c, K] = var[c, h]
            ncomp[c] = K + 1
    return w, mu, var, ncomp


def block_kinds(graph):
    """The kind of every block: -1 mandatory, 0 optional at block index 0, 2 optional at the last block index, 1 any other optional
    block (`sp`)."""
    blocks = graph["blocks"]
    return np.array([-1 if not b[2] else 0 if k == 0 else 2 if k == len(blocks) - 1 else 1 for k, b in enumerate(blocks)], np.int64)


def _block_starts(graph):
    """The first state of every block, in block order."""
    block = np.asarray(graph["block"])
    return np.nonzero(np.concatenate([[True], block[1:] != block[:-1]]))[0]


def arc_costs(graph, loop, opt):
    """The arc costs of the module docstring for one graph from the tables loop (n_classes,) and opt (3,) -> (w (3, J): self, next,
    skip into state j; edge (4,): start in state 0, start in alt[0], end in state J - 1, end in alt[1]), float64 log-probabilities."""
    sid, skip, block = (np.asarray(graph[k], np.int64) for k in ("sid", "skip", "block"))
    loop, opt = np.asarray(loop, np.float64), np.asarray(opt, np.float64)
    J, kind, alt = len(sid), block_kinds(graph), graph["alt"]
    stay, leave, take, pass_ = np.log(loop[sid]), np.log(1.0 - loop[sid]), np.log(opt), np.log(1.0 - opt)
    w = np.zeros((3, J))
    w[0] = stay
    w[1, 1:] = leave[:-1]
    first = np.zeros(J, bool)
    first[_block_starts(graph)] = True
    enter = first & (kind[block] >= 0)
    enter[0] = False                                                       # block 0 is entered by the start edge
    w[1, enter] += take[kind[block[enter]]]
    has = skip >= 0
    w[2, has] = leave[skip[has]] + pass_[kind[block[has] - 1]]
    edge = np.array([take[0] if kind[0] == 0 else 0.0, pass_[0], leave[J - 1], leave[alt[1]] + pass_[2] if alt[1] >= 0 else 0.0])
    return w, edge


def trans_step(n, s, enter, skipped, loop, opt):
    """The transition update of the module docstring: n, s (C,) the class occupancies and the class sums of xi[:, self]; enter, skipped
    (3,) the masses per kind of optional block -> (loop, opt).  A class with n < 1 and a kind with enter + skipped < 1 keep their
    values; every estimate is clipped to [TRANS_FLOOR, 1 - TRANS_FLOOR]."""
    n, s, enter, skipped = (np.asarray(v, np.float64) for v in (n, s, enter, skipped))
    ok = n >= 1.0
    new_loop = np.where(ok, np.clip(s / np.where(ok, n, 1.0), TRANS_FLOOR, 1.0 - TRANS_FLOOR), loop)
    tot = enter + skipped
    ok = tot >= 1.0
    new_opt = np.where(ok, np.clip(enter / np.where(ok, tot, 1.0), TRANS_FLOOR, 1.0 - TRANS_FLOOR), opt)
    return new_loop, new_opt


# ------------------------------------------------------------------------------------------------ TextGrid
def write_textgrid(path, words, phones, xmax):
    """Long Praat text format, IntervalTiers `words` and `phones` of (start, end, text) intervals; times are written with repr, so
    `preprocess.read_textgrid` returns them unchanged."""
    def tier(i, name, items):
        out = [f"    item [{i}]:", '        class = "IntervalTier"', f'        name = "{name}"', "        xmin = 0",
               f"        xmax = {float(xmax)!r}", f"        intervals: size = {len(items)}"]
        for k, (s, e, text) in enumerate(items, 1):
            text = text.replace('"', '""')
            out += [f"        intervals [{k}]:", f"            xmin = {float(s)!r}", f"            xmax = {float(e)!r}",
                    f'            text = "{text}"']
        return out
    lines = ['File type = "ooTextFile"', 'Object class = "TextGrid"', "", "xmin = 0", f"xmax = {float(xmax)!r}", "tiers? <exists>",
             "size = 2", "item []:"] + tier(1, "words", words) + tier(2, "phones", phones)
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


def intervals(graph, words, frames, hop_length, sampling_rate):
    """frames per block -> (words tier, phones tier, xmax): silences are "" in the words tier, zero-frame blocks are left out."""
    t = lambda f: f * hop_length / sampling_rate                          # noqa: E731
    ph, wd, f0 = [], [], 0
    for (p, w, _), n in zip(graph["blocks"], frames):
        n = int(n)
        if n == 0:
            continue
        ph.append((t(f0), t(f0 + n), p))
        if wd and w >= 0 and wd[-1][3] == w:
            wd[-1] = (wd[-1][0], t(f0 + n), wd[-1][2], w)
        else:
            wd.append((t(f0), t(f0 + n), words[w] if w >= 0 else "", w))
        f0 += n
    return [x[:3] for x in wd], ph, t(f0)


# ------------------------------------------------------------------------------------------------ kernels
def max_states():
    return _lib.load().fs2_align_max_states()


def max_mixtures():
    return _lib.load().fs2_align_max_mixtures()


def _dev(t, dtype, what, dim=3):
    ragged.require_device(t, "fastspeech2_amd.align")
    if t.dtype != dtype or t.dim() != dim or (t.numel() and t.stride(-1) != 1):
        raise ValueError(f"{what} must be a {dim}-D {dtype} tensor with unit inner stride, got {t.dtype} {tuple(t.shape)}")
    return t


def _out(out, shape, device, least=(1,), alloc=None, what="out", dtype=torch.float64):
    """The `out=` of a wrapper: a fresh buffer of shape `alloc` (default `shape`), or `out` checked against `shape`, where the
    dimensions listed in `least` may be larger."""
    if out is None:
        return torch.empty(alloc or tuple(shape), dtype=dtype, device=device)
    out = _dev(out, dtype, what, len(shape))
    if any(got < n if d in least else got != n for d, (got, n) in enumerate(zip(out.shape, shape))):
        want = ", ".join(f">= {n}" if d in least else str(n) for d, n in enumerate(shape))
        raise ValueError(f"{what} {tuple(out.shape)} is not ({want})")
    return out


class Graphs:
    """The graphs of one ragged batch on the device: sid / skip / block [B][Jmax] int32 (-1 padded), alt [B][2], jlens."""

    def __init__(self, graphs, device):
        self.graphs = graphs
        self.jl = [len(g["sid"]) for g in graphs]
        self.Jmax = max(self.jl) if graphs else 0
        if self.Jmax > max_states():
            raise ValueError(f"an utterance of {self.Jmax} states exceeds the supported maximum of {max_states()}")
        self.nbmax = max((len(g["blocks"]) for g in graphs), default=0)
        packed = np.full((3, len(graphs), max(self.Jmax, 1)), -1, np.int32)
        for b, g in enumerate(graphs):
            for i, k in enumerate(("sid", "skip", "block")):
                packed[i, b, :self.jl[b]] = g[k]
        self.sid, self.skip, self.block = _up(packed, device)
        self.alt = torch.tensor([g["alt"] for g in graphs], dtype=torch.int32, device=device).reshape(-1, 2)
        self.jlens = torch.tensor(self.jl, dtype=torch.int32, device=device)
        self.ldg = max(self.Jmax, 1)
        self.w, self.edge, self._arc_index = None, None, {}

    def set_arcs(self, loop, opt):
        """The padded device copies w (B, 3, ldg) and edge (B, 4) of every graph's `arc_costs` (0 in the padding); rebuilt after each
        update of the tables."""
        w, edge = np.zeros((len(self.graphs), 3, self.ldg)), np.zeros((len(self.graphs), 4))
        for b, g in enumerate(self.graphs):
            w[b, :, :self.jl[b]], edge[b] = arc_costs(g, loop, opt)
        self.w, self.edge = _up(w, self.sid.device), _up(edge, self.sid.device)

    def arc_index(self, n_classes):
        """The two CSR lists that reduce the arc posteriors xi (B, ldg, 5): the class list of `index` and the list of the optional
        blocks, row classes (kind 0 enter, skipped, kind 1 enter, skipped, kind 2 enter, skipped) as the module docstring names the
        states, utterances then blocks ascending.  Cached per number of classes."""
        if n_classes not in self._arc_index:
            rows = [[] for _ in range(6)]
            for b, g in enumerate(self.graphs):
                first, at = _block_starts(g), b * self.ldg
                for k, kind in enumerate(block_kinds(g)):
                    if kind == 0:
                        rows[0].append(at), rows[1].append(at + g["alt"][0])
                    elif kind == 1:
                        rows[2].append(at + first[k]), rows[3].append(at + first[k + 1])
                    elif kind == 2:
                        rows[4].append(at + first[k]), rows[5].append(at + g["alt"][1])
            kinds = _csr(np.repeat(np.arange(6), [len(r) for r in rows]), 6, self.sid.device, [i for r in rows for i in r])
            self._arc_index[n_classes] = (self.index(n_classes, self.ldg), kinds)
        return self._arc_index[n_classes]

    def index(self, n_classes, ld_j, mixtures=1):
        """CSR (class -> rows b * ld_j + j of the partials), utterances then states ascending: (offs, items) on the device.  With
        `mixtures` = M > 1 the row classes are c * M + m and the rows (b * ld_j + j) * M + m, in the same order within a row class."""
        cls = np.concatenate([g["sid"].astype(np.int64) for g in self.graphs]) if self.graphs else np.zeros(0, np.int64)
        rows = np.concatenate([b * ld_j + np.arange(n, dtype=np.int64) for b, n in enumerate(self.jl)]) if self.graphs \
            else np.zeros(0, np.int64)
        if cls.size and (cls.min() < 0 or cls.max() >= n_classes):
            raise ValueError(f"emission class outside [0, {n_classes})")
        if mixtures > 1:
            comp = np.arange(mixtures, dtype=np.int64)[None, :]
            cls, rows = (cls[:, None] * mixtures + comp).ravel(), (rows[:, None] * mixtures + comp).ravel()
            n_classes *= mixtures
        return _csr(cls, n_classes, self.sid.device, rows)


def _check_scan(E, lens, G):
    E = _dev(E, torch.float64, "E")
    B, Tmax, Jmax = E.shape
    if B != len(G.jl) or Jmax < G.Jmax:
        raise ValueError(f"E {tuple(E.shape)} does not hold {len(G.jl)} utterances of up to {G.Jmax} states")
    lens_h, lens_d = ragged.lengths(lens, B, Tmax, "lens", E.device)
    return E, B, Tmax, lens_h, lens_d


def features(mel, lens):
    """mel (B, n_mel, frames) float32 log-mel on the device, lens frames per row -> x (B, Tmax, 2 n_mel) float64."""
    mel = _dev(mel, torch.float32, "mel")
    B, n_mel, F = mel.shape
    lens_h, lens_d = ragged.lengths(lens, B, F, "lens", mel.device)
    Tmax = max(lens_h, default=0)
    x = torch.empty(B, Tmax, 2 * n_mel, dtype=torch.float64, device=mel.device)
    mean = torch.empty(B, n_mel, dtype=torch.float64, device=mel.device)
    _lib.call("fs2_align_feats", mel.data_ptr(), mel.stride(0), mel.stride(1), lens_d.data_ptr(), mean.data_ptr(), x.data_ptr(),
              x.stride(0), x.stride(1), B, n_mel, Tmax, ops._stream())
    return x


def emit(x, lens, G, mu, var, out=None):
    """E (B, Tmax, Jmax) float64 from features x (B, Tmax, D), the batch's Graphs and the class tables mu, var (C, D)."""
    x = _dev(x, torch.float64, "x")
    mu, var = _dev(mu, torch.float64, "mu", 2).contiguous(), _dev(var, torch.float64, "var", 2).contiguous()
    B, Tmax, D = x.shape
    if mu.shape != var.shape or mu.shape[1] != D or B != len(G.jl):
        raise ValueError(f"x {tuple(x.shape)}, mu {tuple(mu.shape)}, var {tuple(var.shape)}, {len(G.jl)} graphs do not fit together")
    _, lens_d = ragged.lengths(lens, B, Tmax, "lens", x.device)
    E = _out(out, (B, Tmax, G.Jmax), x.device, least=(1, 2))
    _lib.call("fs2_align_emit", x.data_ptr(), x.stride(0), x.stride(1), lens_d.data_ptr(), G.jlens.data_ptr(), G.sid.data_ptr(), G.ldg,
              mu.data_ptr(), var.data_ptr(), mu.shape[0], D, E.data_ptr(), E.stride(0), E.stride(1), B, Tmax, G.Jmax, ops._stream())
    return E


def _no_host(**tensors):
    for what, t in tensors.items():
        if t is not None and (not isinstance(t, torch.Tensor) or t.device.type != "cuda"):
            raise ValueError(f"{what} must be a tensor on the GPU (fastspeech2_amd.align has no CPU fallback)")


def _check_mix(w, mu, var, D):
    w = _dev(w, torch.float64, "w", 2).contiguous()
    mu, var = _dev(mu, torch.float64, "mu", 3).contiguous(), _dev(var, torch.float64, "var", 3).contiguous()
    M = w.shape[1]
    if not 1 <= M <= max_mixtures():
        raise ValueError(f"{M} mixture components, supported are 1..{max_mixtures()}")
    if mu.shape != var.shape or mu.shape[:2] != w.shape or mu.shape[2] != D or w.shape[0] == 0:
        raise ValueError(f"w {tuple(w.shape)}, mu {tuple(mu.shape)}, var {tuple(var.shape)} and D = {D} do not fit together")
    return w, mu, var, M


def emit_gmm(x, lens, G, w, mu, var, out=None, resp=None):
    """E (B, Tmax, Jmax) float64 from the mixture tables w (C, M), mu, var (C, M, D); responsibilities are written to `resp`
    (B, >= Tmax, >= Jmax, M) when it is given (decoding passes none)."""
    _no_host(x=x, w=w, mu=mu, var=var, out=out, resp=resp)
    x = _dev(x, torch.float64, "x")
    B, Tmax, D = x.shape
    w, mu, var, M = _check_mix(w, mu, var, D)
    if B != len(G.jl):
        raise ValueError(f"x {tuple(x.shape)} and {len(G.jl)} graphs do not fit together")
    _, lens_d = ragged.lengths(lens, B, Tmax, "lens", x.device)
    E = _out(out, (B, Tmax, G.Jmax), x.device, least=(1, 2))
    rp, rs = None, (0, 0, 0)
    if resp is not None:
        resp = _dev(resp, torch.float64, "resp", 4)
        if resp.shape[0] != B or resp.shape[1] < Tmax or resp.shape[2] < G.Jmax or resp.shape[3] != M:
            raise ValueError(f"resp {tuple(resp.shape)} is not ({B}, >= {Tmax}, >= {G.Jmax}, {M})")
        rp, rs = resp.data_ptr(), resp.stride()[:3]
    _lib.call("fs2_align_emit_gmm", x.data_ptr(), x.stride(0), x.stride(1), lens_d.data_ptr(), G.jlens.data_ptr(), G.sid.data_ptr(),
              G.ldg, w.data_ptr(), mu.data_ptr(), var.data_ptr(), w.shape[0], M, D, E.data_ptr(), E.stride(0), E.stride(1), rp, rs[0],
              rs[1], rs[2], B, Tmax, G.Jmax, ops._stream())
    return E


def _arc_args(w, edge, B, G):
    """The suffix of a scan's entry point and the arguments it takes more under the arc costs w (B, 3, >= Jmax) and edge (B, 4):
    ("", ()) without costs, else ("_arcs", (w, its row stride, edge)) after the checks."""
    if w is None and edge is None:
        return "", ()
    if w is None or edge is None:
        raise ValueError("w and edge are given together or not at all")
    _no_host(w=w, edge=edge)
    w, edge = _dev(w, torch.float64, "w"), _dev(edge, torch.float64, "edge", 2)
    if w.shape[0] != B or w.shape[1] != 3 or w.shape[2] < G.Jmax or (B and w.stride(0) != 3 * w.stride(1)) or \
            tuple(edge.shape) != (B, 4) or not edge.is_contiguous():
        raise ValueError(f"w {tuple(w.shape)} (strides {w.stride()}) and edge {tuple(edge.shape)} are not the arc costs [B][3][ldw] and "
                         f"[B][4] of {B} utterances of up to {G.Jmax} states")
    return "_arcs", (w.data_ptr(), w.stride(1), edge.data_ptr())


def forward(E, lens, G, out=None, w=None, edge=None):
    """-> (alpha like E, loglik (B,)) on the device; under the arc costs w, edge when they are given."""
    E, B, Tmax, _, lens_d = _check_scan(E, lens, G)
    arcs, costs = _arc_args(w, edge, B, G)
    alpha = _out(out, E.shape, E.device, least=())
    loglik = torch.empty(B, dtype=torch.float64, device=E.device)
    _lib.call("fs2_align_forward" + arcs, E.data_ptr(), E.stride(0), E.stride(1), lens_d.data_ptr(), G.jlens.data_ptr(),
              G.skip.data_ptr(), G.ldg, G.alt.data_ptr(), *costs, alpha.data_ptr(), alpha.stride(0), alpha.stride(1), loglik.data_ptr(),
              B, Tmax, G.Jmax, ops._stream())
    return alpha, loglik


def backward(E, lens, G, alpha, loglik, out=None, w=None, edge=None, xi=None):
    """gamma = exp(alpha + beta - loglik), written over alpha unless `out` is given.  Under the arc costs w, edge -> (gamma, xi
    (B, >= Jmax, 5): the arc posteriors self, next, skip of every state, then its start mass gamma[0, j] and its end mass
    gamma[T - 1, j])."""
    E, B, Tmax, _, lens_d = _check_scan(E, lens, G)
    arcs, costs = _arc_args(w, edge, B, G)
    alpha = _dev(alpha, torch.float64, "alpha")
    gamma = alpha if out is None else _dev(out, torch.float64, "out")
    loglik = _dev(loglik, torch.float64, "loglik", 1)
    if alpha.shape != E.shape or gamma.shape != E.shape or loglik.shape[0] != B:
        raise ValueError("alpha and out must have E's shape, loglik B values")
    sums = ()
    if arcs:
        xi = _out(xi, (B, G.Jmax, 5), E.device, alloc=(B, G.ldg, 5), what="xi")
        sums = (xi.data_ptr(), xi.stride(0), xi.stride(1))
    _lib.call("fs2_align_backward" + arcs, E.data_ptr(), E.stride(0), E.stride(1), lens_d.data_ptr(), G.jlens.data_ptr(),
              G.skip.data_ptr(), G.ldg, G.alt.data_ptr(), *costs, alpha.data_ptr(), alpha.stride(0), alpha.stride(1), loglik.data_ptr(),
              gamma.data_ptr(), gamma.stride(0), gamma.stride(1), *sums, B, Tmax, G.Jmax, ops._stream())
    return (gamma, xi) if arcs else gamma


def forward_arcs(E, lens, G, w, edge, out=None):
    """`forward` under the arc costs w (B, 3, >= Jmax) and edge (B, 4)."""
    return forward(E, lens, G, out, w, edge)


def backward_arcs(E, lens, G, w, edge, alpha, loglik, out=None, xi=None):
    """`backward` under the arc costs -> (gamma, xi)."""
    return backward(E, lens, G, alpha, loglik, out, w, edge, xi)


def stats(gamma, x, lens, G, out=None):
    """Per-utterance partials (B, Jmax, 1 + 2 D)."""
    gamma, B, Tmax, _, lens_d = _check_scan(gamma, lens, G)
    x = _dev(x, torch.float64, "x")
    D = x.shape[2]
    if x.shape[0] != B or x.shape[1] < Tmax:
        raise ValueError(f"x {tuple(x.shape)} does not cover gamma {tuple(gamma.shape)}")
    P = _out(out, (B, G.Jmax, 1 + 2 * D), x.device, alloc=(B, G.ldg, 1 + 2 * D))
    _lib.call("fs2_align_stats", gamma.data_ptr(), gamma.stride(0), gamma.stride(1), x.data_ptr(), x.stride(0), x.stride(1),
              lens_d.data_ptr(), G.jlens.data_ptr(), D, P.data_ptr(), P.stride(0), P.stride(1), B, Tmax, G.Jmax, ops._stream())
    return P


def stats_gmm(gamma, resp, x, lens, G, out=None):
    """Per-utterance mixture partials (B, Jmax, M, 1 + 2 D) of gamma (B, T, J) and the responsibilities resp (B, T, J, M)."""
    _no_host(gamma=gamma, resp=resp, x=x, out=out)
    gamma, B, Tmax, _, lens_d = _check_scan(gamma, lens, G)
    x, resp = _dev(x, torch.float64, "x"), _dev(resp, torch.float64, "resp", 4)
    D, M = x.shape[2], resp.shape[3]
    if not 1 <= M <= max_mixtures():
        raise ValueError(f"{M} mixture components, supported are 1..{max_mixtures()}")
    if x.shape[0] != B or x.shape[1] < Tmax:
        raise ValueError(f"x {tuple(x.shape)} does not cover gamma {tuple(gamma.shape)}")
    if resp.shape[0] != B or resp.shape[1] < Tmax or resp.shape[2] < G.Jmax:
        raise ValueError(f"resp {tuple(resp.shape)} does not cover gamma {tuple(gamma.shape)}")
    P = torch.empty(B, G.ldg, M, 1 + 2 * D, dtype=torch.float64, device=x.device) if out is None \
        else _dev(out, torch.float64, "out", 4)
    if P.shape[0] != B or P.shape[1] < G.Jmax or P.shape[2] != M or P.shape[3] != 1 + 2 * D or P.stride(1) != M * P.stride(2):
        raise ValueError(f"out {tuple(P.shape)} is not ({B}, >= {G.Jmax}, {M}, {1 + 2 * D}) with the components of a state together")
    _lib.call("fs2_align_stats_gmm", gamma.data_ptr(), gamma.stride(0), gamma.stride(1), resp.data_ptr(), resp.stride(0),
              resp.stride(1), resp.stride(2), x.data_ptr(), x.stride(0), x.stride(1), lens_d.data_ptr(), G.jlens.data_ptr(), M, D,
              P.data_ptr(), P.stride(0), P.stride(2), B, Tmax, G.Jmax, ops._stream())
    return P


def reduce(P, G, n_classes, sums=None, index=None):
    """Class sums (C, 1 + 2 D) of the partials; added to `sums` when given.  Mixture partials (B, J, M, 1 + 2 D) give (C M, 1 + 2 D),
    component m of class c in row c M + m."""
    if P.dim() == 4:
        if not P.is_contiguous():
            raise ValueError("partials must be contiguous")
        M = P.shape[2]
        index = index if index is not None else G.index(n_classes, P.shape[1], M)
        return reduce(P.view(P.shape[0], P.shape[1] * M, P.shape[3]), G, n_classes * M, sums, index)
    P = _dev(P, torch.float64, "partials")
    if not P.is_contiguous():
        raise ValueError("partials must be contiguous")
    offs, items = index if index is not None else G.index(n_classes, P.shape[1])
    acc = sums is not None
    if sums is None:
        sums = torch.empty(n_classes, P.shape[2], dtype=torch.float64, device=P.device)
    _lib.call("fs2_align_reduce", P.data_ptr(), P.stride(1), P.shape[0] * P.shape[1], offs.data_ptr(), items.data_ptr(), n_classes,
              P.shape[2], sums.data_ptr(), int(acc), ops._stream())
    return sums


def max_splice_dim():
    return _lib.load().fs2_align_max_splice_dim()


def splice_dim(n_mel, context, k=None):
    """D_s = n_mel (2 c + 1) after the checks of the module docstring: c in 0..4, D_s <= `max_splice_dim()`, 1 <= k <= D_s."""
    n_mel, context = int(n_mel), int(context)
    if not 0 <= context <= 4:
        raise ValueError(f"splice must be 0..4 frames of context, got {context}")
    Ds = n_mel * (2 * context + 1)
    if n_mel < 1 or Ds > max_splice_dim():
        raise ValueError(f"{n_mel} channels x {2 * context + 1} frames = {Ds} spliced dimensions, supported are 1..{max_splice_dim()}")
    if k is not None and not 1 <= int(k) <= Ds:
        raise ValueError(f"lda must be 1..{Ds} output dimensions (D_s), got {k}")
    return Ds


def splice(x, lens, n_mel, context, out=None):
    """y (B, Tmax, n_mel (2 c + 1)) float64: the first n_mel columns of x (B, Tmax, >= n_mel) over the frames t - c .. t + c, clamped
    at each utterance's own ends."""
    _no_host(x=x, out=out)
    x = _dev(x, torch.float64, "x")
    B, Tmax, D = x.shape
    Ds = splice_dim(n_mel, context)
    if D < n_mel:
        raise ValueError(f"x {tuple(x.shape)} has fewer than {n_mel} columns")
    _, lens_d = ragged.lengths(lens, B, Tmax, "lens", x.device)
    y = _out(out, (B, Tmax, Ds), x.device)
    _lib.call("fs2_align_splice", x.data_ptr(), x.stride(0), x.stride(1), lens_d.data_ptr(), int(n_mel), int(context), y.data_ptr(),
              y.stride(0), y.stride(1), B, Tmax, ops._stream())
    return y


def scatter(y, lens, s=None, S=None):
    """(s (D_s,), S (D_s, D_s)) float64 on the device: sum y and sum y y^T over the valid frames of the batch, added to `s` and `S`
    when they are given (both or neither).  S is exactly symmetric."""
    _no_host(y=y, s=s, S=S)
    y = _dev(y, torch.float64, "y")
    B, Tmax, Ds = y.shape
    if not 1 <= Ds <= max_splice_dim():
        raise ValueError(f"{Ds} dimensions, supported are 1..{max_splice_dim()}")
    if (s is None) != (S is None):
        raise ValueError("s and S are given together or not at all")
    if s is None:
        s = torch.zeros(Ds, dtype=torch.float64, device=y.device)
        S = torch.zeros(Ds, Ds, dtype=torch.float64, device=y.device)
    s, S = _dev(s, torch.float64, "s", 1), _dev(S, torch.float64, "S", 2)
    if s.shape[0] != Ds or tuple(S.shape) != (Ds, Ds):
        raise ValueError(f"s {tuple(s.shape)} and S {tuple(S.shape)} do not fit y {tuple(y.shape)}")
    _, lens_d = ragged.lengths(lens, B, Tmax, "lens", y.device)
    n_ws = _lib.load().fs2_align_scatter_ws(B, Tmax, Ds)
    ws = torch.empty(max(n_ws, 1), dtype=torch.float64, device=y.device)
    _lib.call("fs2_align_scatter", y.data_ptr(), y.stride(0), y.stride(1), lens_d.data_ptr(), Ds, s.data_ptr(), S.data_ptr(), S.stride(0),
              ws.data_ptr(), n_ws, B, Tmax, ops._stream())
    return s, S


def project(y, lens, P, o, out=None):
    """z (B, Tmax, k) float64 = P y - o for P (k, D_s), o (k,) on the device."""
    _no_host(y=y, P=P, o=o, out=out)
    y = _dev(y, torch.float64, "y")
    P, o = _dev(P, torch.float64, "P", 2).contiguous(), _dev(o, torch.float64, "o", 1).contiguous()
    B, Tmax, Ds = y.shape
    k = P.shape[0]
    if P.shape[1] != Ds or o.shape[0] != k:
        raise ValueError(f"y {tuple(y.shape)}, P {tuple(P.shape)} and o {tuple(o.shape)} do not fit together")
    if not 1 <= k <= Ds <= max_splice_dim():
        raise ValueError(f"{k} outputs of {Ds} dimensions, supported are 1 <= k <= D_s <= {max_splice_dim()}")
    _, lens_d = ragged.lengths(lens, B, Tmax, "lens", y.device)
    z = _out(out, (B, Tmax, k), y.device)
    _lib.call("fs2_align_project", y.data_ptr(), y.stride(0), y.stride(1), lens_d.data_ptr(), P.data_ptr(), o.data_ptr(), k, Ds,
              z.data_ptr(), z.stride(0), z.stride(1), B, Tmax, ops._stream())
    return z


def lda_transform(n, a, N, s, S, k):
    """The transform of the module docstring from the class sums n (C,), a (C, D_s) and the totals N, s (D_s,), S (D_s, D_s)
    -> (P (k, D_s), o (k,), the k eigenvalues in descending order), numpy float64."""
    n, a, s, S = (np.asarray(v, np.float64) for v in (n, a, s, S))
    Ds = s.shape[0]
    if a.ndim != 2 or a.shape != (n.shape[0], Ds) or S.shape != (Ds, Ds):
        raise ValueError(f"n {n.shape}, a {a.shape}, s {s.shape} and S {S.shape} do not fit together")
    if not 1 <= int(k) <= Ds:
        raise ValueError(f"lda must be 1..{Ds} output dimensions (D_s), got {k}")
    if not N > 0:
        raise ValueError("no frames")
    m = s / N
    S_T = S / N - np.outer(m, m)
    ok = n >= 1.0
    d = a[ok] / n[ok, None] - m[None, :]
    S_B = (d * n[ok, None]).T @ d / N
    S_B = 0.5 * (S_B + S_B.T)
    S_W = S_T - S_B + (1e-8 * np.trace(S_T) / Ds) * np.eye(Ds)
    L = np.linalg.cholesky(0.5 * (S_W + S_W.T))
    M = np.linalg.solve(L, np.linalg.solve(L, S_B).T)                      # L^-1 S_B L^-T (S_B is symmetric)
    w, V = np.linalg.eigh(0.5 * (M + M.T))
    top = np.argsort(-w, kind="stable")[:int(k)]
    P = np.linalg.solve(L.T, V[:, top]).T                                  # rows v^T L^-1
    lead = np.argmax(np.abs(P), axis=1)                                    # the first of the largest
    P = P * np.where(P[np.arange(len(P)), lead] < 0.0, -1.0, 1.0)[:, None]
    return P, P @ m, w[top]


def max_fmllr_dim():
    return _lib.load().fs2_align_max_fmllr_dim()


def _fmllr_dim(D, what="fmllr"):
    if not 1 <= int(D) <= max_fmllr_dim():
        raise ValueError(f"{what}: {D} feature dimensions, supported are 1..{max_fmllr_dim()}")
    return int(D)


def _speaker_list(speakers, B, n_spk):
    sp = np.asarray(list(speakers), dtype=np.int64).reshape(-1) if speakers is not None else None
    if sp is None or sp.shape[0] != B:
        raise ValueError(f"speakers must hold one speaker index for each of the {B} utterances")
    if sp.size and (sp.min() < 0 or sp.max() >= n_spk):
        raise ValueError(f"speaker index outside [0, {n_spk})")
    return sp


def fmllr_weights(gamma, lens, G, mu, var, out=None):
    """The frame weights (c, h), each (B, Tmax, D) float64, from the posteriors gamma (B, Tmax, Jmax), the batch's Graphs and the
    class tables mu, var (C, D); `out` = (c, h) may give the buffers."""
    _no_host(gamma=gamma, mu=mu, var=var)
    gamma, B, Tmax, _, lens_d = _check_scan(gamma, lens, G)
    mu, var = _dev(mu, torch.float64, "mu", 2).contiguous(), _dev(var, torch.float64, "var", 2).contiguous()
    D = _fmllr_dim(mu.shape[1], "fmllr_weights")
    if mu.shape != var.shape or mu.shape[0] == 0:
        raise ValueError(f"mu {tuple(mu.shape)} and var {tuple(var.shape)} do not fit together")
    if out is None:
        out = (torch.empty(B, Tmax, D, dtype=torch.float64, device=gamma.device), torch.empty(B, Tmax, D, dtype=torch.float64, device=gamma.device))
    _no_host(c=out[0], h=out[1])
    c, h = _dev(out[0], torch.float64, "c"), _dev(out[1], torch.float64, "h")
    if c.shape[0] != B or c.shape[1] < Tmax or c.shape[2] != D or c.shape != h.shape or c.stride() != h.stride():
        raise ValueError(f"out {tuple(c.shape)}, {tuple(h.shape)} is not twice ({B}, >= {Tmax}, {D}) with the same strides")
    _lib.call("fs2_align_fmllr_weights", gamma.data_ptr(), gamma.stride(0), gamma.stride(1), lens_d.data_ptr(), G.jlens.data_ptr(),
              G.sid.data_ptr(), G.ldg, mu.data_ptr(), var.data_ptr(), mu.shape[0], D, c.data_ptr(), h.data_ptr(), c.stride(0), c.stride(1),
              B, Tmax, G.Jmax, ops._stream())
    return c, h


def fmllr_accumulate(f, c, h, lens, speakers, n_spk, beta=None, G=None, k=None):
    """(beta (n_spk,), G (n_spk, D, D + 1, D + 1), k (n_spk, D, D + 1)) float64 on the device: the speaker statistics of one batch
    from the unadapted features f and the frame weights c, h (all (B, Tmax, D)), `speakers` one index per utterance (host); added
    to `beta`, `G`, `k` when they are given (all or none).  G[s, i] is exactly symmetric; a speaker without utterances in the batch
    keeps its tables."""
    _no_host(f=f, c=c, h=h, beta=beta, G=G, k=k)
    f, c, h = _dev(f, torch.float64, "f"), _dev(c, torch.float64, "c"), _dev(h, torch.float64, "h")
    B, Tmax, D = f.shape
    _fmllr_dim(D, "fmllr_accumulate")
    if c.shape[0] != B or c.shape[1] < Tmax or c.shape[2] != D or c.shape != h.shape or c.stride() != h.stride():
        raise ValueError(f"c {tuple(c.shape)} and h {tuple(h.shape)} do not fit f {tuple(f.shape)}")
    n_spk = int(n_spk)
    if n_spk < 1:
        raise ValueError(f"n_spk must be at least 1, got {n_spk}")
    sp = _speaker_list(speakers, B, n_spk)
    if (beta is None) != (G is None) or (beta is None) != (k is None):
        raise ValueError("beta, G and k are given together or not at all")
    if beta is None:
        beta = torch.zeros(n_spk, dtype=torch.float64, device=f.device)
        G = torch.zeros(n_spk, D, D + 1, D + 1, dtype=torch.float64, device=f.device)
        k = torch.zeros(n_spk, D, D + 1, dtype=torch.float64, device=f.device)
    beta, G, k = _dev(beta, torch.float64, "beta", 1), _dev(G, torch.float64, "G", 4), _dev(k, torch.float64, "k", 3)
    if tuple(beta.shape) != (n_spk,) or tuple(G.shape) != (n_spk, D, D + 1, D + 1) or tuple(k.shape) != (n_spk, D, D + 1) or \
            not (beta.is_contiguous() and G.is_contiguous() and k.is_contiguous()):
        raise ValueError(f"beta {tuple(beta.shape)}, G {tuple(G.shape)}, k {tuple(k.shape)} are not the contiguous tables of {n_spk} "
                         f"speakers in {D} dimensions")
    _, lens_d = ragged.lengths(lens, B, Tmax, "lens", f.device)
    offs_d, rows_d = _csr(sp, n_spk, f.device)                             # speaker -> batch rows, in batch-row order
    n_ws = _lib.load().fs2_align_fmllr_accum_ws(B, Tmax, D)
    ws = torch.empty(max(n_ws, 1), dtype=torch.float64, device=f.device)
    _lib.call("fs2_align_fmllr_accum", f.data_ptr(), f.stride(0), f.stride(1), c.data_ptr(), h.data_ptr(), c.stride(0), c.stride(1),
              lens_d.data_ptr(), offs_d.data_ptr(), rows_d.data_ptr(), n_spk, D, beta.data_ptr(), G.data_ptr(), k.data_ptr(),
              ws.data_ptr(), n_ws, B, Tmax, ops._stream())
    return beta, G, k


def fmllr_apply(f, lens, W, speakers, out=None):
    """fh (B, Tmax, D) float64 = W[speaker] (f, 1) for W (n_spk, D, D + 1) on the device, `speakers` one index per utterance (host)."""
    _no_host(f=f, W=W, out=out)
    f, W = _dev(f, torch.float64, "f"), _dev(W, torch.float64, "W").contiguous()
    B, Tmax, D = f.shape
    _fmllr_dim(D, "fmllr_apply")
    if W.shape[0] < 1 or tuple(W.shape[1:]) != (D, D + 1):
        raise ValueError(f"W {tuple(W.shape)} is not (n_spk, {D}, {D + 1})")
    sp = _speaker_list(speakers, B, W.shape[0])
    _, lens_d = ragged.lengths(lens, B, Tmax, "lens", f.device)
    fh = _out(out, (B, Tmax, D), f.device)
    spk_d = _up(sp.astype(np.int32), f.device)
    _lib.call("fs2_align_fmllr_apply", f.data_ptr(), f.stride(0), f.stride(1), lens_d.data_ptr(), W.data_ptr(), spk_d.data_ptr(),
              W.shape[0], D, fh.data_ptr(), fh.stride(0), fh.stride(1), B, Tmax, ops._stream())
    return fh


def fmllr_update(beta, G, k, W, min_frames=500.0, sweeps=20, trace=None):
    """The update of the module docstring for all speakers at once: beta (S,), G (S, D, D + 1, D + 1), k (S, D, D + 1) and the current
    W (S, D, D + 1) -> (W, status (S,) int8: 0 adapted, 1 kept for too few frames, 2 kept because a G_s[i] is not positive
    definite), numpy float64.  `trace`, a list, receives a copy of the adapted speakers' W after every row step (the tests)."""
    beta, G, k, W = (np.array(v, dtype=np.float64) for v in (beta, G, k, W))
    if k.ndim != 3 or k.shape[2] != k.shape[1] + 1 or G.shape != k.shape + (k.shape[2],) or W.shape != k.shape or beta.shape != k.shape[:1]:
        raise ValueError(f"beta {beta.shape}, G {G.shape}, k {k.shape} and W {W.shape} do not fit together")
    S, D, P = k.shape
    status = np.where(beta < min_frames, 1, 0).astype(np.int8)
    Gi = np.zeros_like(G)
    for s in np.nonzero(status == 0)[0]:
        try:
            np.linalg.cholesky(G[s])
            Gi[s] = np.linalg.inv(G[s])
        except np.linalg.LinAlgError:
            status[s] = 2
    ok = np.nonzero(status == 0)[0]
    if ok.size == 0:
        return W, status
    Gi, kk, b, Wk = Gi[ok], k[ok], beta[ok], W[ok]
    for _ in range(int(sweeps)):
        for i in range(D):
            p = np.concatenate([np.linalg.inv(Wk[:, :, :D])[:, :, i], np.zeros((len(ok), 1))], axis=1)
            pG = np.einsum("np,npq->nq", p, Gi[:, i])
            a, c = np.einsum("nq,nq->n", pG, p), np.einsum("nq,nq->n", pG, kk[:, i])
            root = np.sqrt(c * c + 4.0 * a * b)
            alpha = [(-c + root) / (2.0 * a), (-c - root) / (2.0 * a)]
            gain = [b * np.log(np.abs(al * a + c)) - 0.5 * a * al * al for al in alpha]
            al = np.where(gain[0] >= gain[1], alpha[0], alpha[1])          # the '+' root on a tie
            Wk[:, i] = np.einsum("np,npq->nq", al[:, None] * p + kk[:, i], Gi[:, i])
            if trace is not None:
                trace.append(Wk.copy())
    W[ok] = Wk
    return W, status


BOUNDARY = "#"


def max_tree_sets():
    return _lib.load().fs2_align_max_tree_sets()


def triphone_contexts(graph, phone_ids, states=2):
    """int32 (J, 4): per state j the ids (l, p, r, s) of its logical state.  l and r are phone ids or `len(phone_ids)`, the id of the
    boundary symbol `#`: the phone of the neighbouring block when that block belongs to the same word, else `#`.  `sil`, `sp` and `spn`
    are context-independent: they have l = r = `#` and are never a context."""
    bnd, ci, blocks = len(phone_ids), (SIL, SP, SPN), graph["blocks"]
    if len(graph["sid"]) != len(blocks) * states:
        raise ValueError(f"a graph of {len(graph['sid'])} states does not have {states} states per block")

    def neighbour(k, other):
        if not 0 <= other < len(blocks) or blocks[k][0] in ci or blocks[k][1] < 0:
            return bnd
        p, w, _ = blocks[other]
        return phone_ids[p] if w == blocks[k][1] and p not in ci else bnd
    out = np.empty((len(blocks) * states, 4), np.int32)
    for k, (p, _, _) in enumerate(blocks):
        for s in range(states):
            out[k * states + s] = (neighbour(k, k - 1), phone_ids[p], neighbour(k, k + 1), s)
    return out


def node_loglik(n, a, q, floor):
    """L(n, a, q) = -n / 2 sum_d (log(2 pi v_d) + 1), v_d = max(q_d / n - (a_d / n)^2, floor_d), d ascending; 0 for n = 0."""
    if not n > 0.0:
        return 0.0
    mu = a / n
    return -0.5 * n * float(np.cumsum(np.log(2.0 * np.pi * np.maximum(q / n - mu * mu, floor)) + 1.0)[-1])


def phone_questions(mono, phones, states, floor, n_symbols):
    """The generated question sets of the module docstring from the pooled monophone sums `mono` (phones x states, 1 + 2 D): bottom-up
    clustering of the real phones `phones` (ids) -> (names, member uint8 (2 P - 1, n_symbols)): the singletons in ascending order,
    the merged sets in merge order without the full set, then `{#}` (symbol n_symbols - 1)."""
    D = (mono.shape[1] - 1) // 2
    phones = sorted(int(p) for p in phones)
    lik = lambda t: sum(node_loglik(t[s, 0], t[s, 1:1 + D], t[s, 1 + D:], floor) for s in range(states))     # noqa: E731
    sets = {p: [p] for p in phones}
    tabs = {p: mono[p * states:(p + 1) * states] for p in phones}
    liks = {p: lik(t) for p, t in tabs.items()}
    cost = lambda i, j: liks[i] + liks[j] - lik(tabs[i] + tabs[j])                                          # noqa: E731
    costs = {(i, j): cost(i, j) for i in phones for j in phones if i < j}
    out = [[p] for p in phones]
    while len(sets) > 2:
        best = None
        for pair in sorted(costs):                                         # the lowest pair on ties
            if best is None or costs[pair] < costs[best]:
                best = pair
        i, j = best
        sets[i], tabs[i] = sorted(sets[i] + sets.pop(j)), tabs[i] + tabs.pop(j)
        liks[i] = lik(tabs[i])
        del liks[j]
        costs = {pr: c for pr, c in costs.items() if i not in pr and j not in pr}
        for o in sets:
            if o != i:
                costs[(min(o, i), max(o, i))] = cost(min(o, i), max(o, i))
        out.append(list(sets[i]))
    out.append([n_symbols - 1])
    member = np.zeros((len(out), n_symbols), np.uint8)
    for k, ids in enumerate(out):
        member[k, ids] = 1
    return [f"g{k}" for k in range(len(out))], member


def read_questions(path, phone_ids):
    """A questions file, one set per line as `name phone phone ...` (`#` is the word boundary) -> (names, member uint8 (n_sets,
    len(phone_ids) + 1)).  An unknown phone or a set without phones is a ValueError."""
    names, rows = [], []
    with open(path, encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) < 2:
                raise ValueError(f"{path}:{no}: the question {parts[0]} names no phone")
            row = np.zeros(len(phone_ids) + 1, np.uint8)
            for p in parts[1:]:
                if p != BOUNDARY and p not in phone_ids:
                    raise ValueError(f"{path}:{no}: unknown phone {p}")
                row[len(phone_ids) if p == BOUNDARY else phone_ids[p]] = 1
            names.append(parts[0])
            rows.append(row)
    if not rows:
        raise ValueError(f"{path} holds no question")
    return names, np.stack(rows)


def tree_gains(sums, left, right, offs, items, member, floor, min_occ, full=False):
    """For every node of the CSR list (offs (n_nodes + 1,), items: int32 indices into the item table `sums` (n_items, 1 + 2 D)) and
    every question of `member` (n_sets, n_symbols) uint8 over the items' context symbols `left`, `right` (n_items,) int32:
    -> (best question (n_nodes,) int32, -1 when no split is eligible; its gain (n_nodes,) float64) and, with `full`, the tables
    gains and n_yes (n_nodes, 2 n_sets).  Everything on the device."""
    _no_host(sums=sums, left=left, right=right, offs=offs, items=items, member=member, floor=floor)
    sums, floor = _dev(sums, torch.float64, "sums", 2), _dev(floor, torch.float64, "floor", 1)
    left, right = _dev(left, torch.int32, "left", 1), _dev(right, torch.int32, "right", 1)
    offs, items = _dev(offs, torch.int32, "offs", 1), _dev(items, torch.int32, "items", 1)
    member = _dev(member, torch.uint8, "member", 2)
    n_items, cols = sums.shape
    D = (cols - 1) // 2
    if cols != 1 + 2 * D or D < 1 or floor.shape[0] != D or left.shape[0] != n_items or right.shape[0] != n_items or offs.shape[0] < 1:
        raise ValueError(f"sums {tuple(sums.shape)}, floor {tuple(floor.shape)}, left {tuple(left.shape)}, right {tuple(right.shape)} and "
                         f"offs {tuple(offs.shape)} do not fit together")
    if not member.is_contiguous() or member.shape[1] < 1:
        raise ValueError(f"member {tuple(member.shape)} must be a contiguous (n_sets, n_symbols) table")
    if not 1 <= member.shape[0] <= max_tree_sets():
        raise ValueError(f"{member.shape[0]} question sets, supported are 1..{max_tree_sets()}")
    if not float(min_occ) >= 1.0:
        raise ValueError(f"tri_min_occ must be at least 1, got {min_occ}")
    n_nodes, Q = offs.shape[0] - 1, 2 * member.shape[0]
    best_q = torch.empty(n_nodes, dtype=torch.int32, device=sums.device)
    best_gain = torch.empty(n_nodes, dtype=torch.float64, device=sums.device)
    gains = torch.empty(n_nodes, Q, dtype=torch.float64, device=sums.device) if full else None
    n_yes = torch.empty(n_nodes, Q, dtype=torch.float64, device=sums.device) if full else None
    _lib.call("fs2_align_tree_gains", sums.data_ptr(), sums.stride(0), n_items, left.data_ptr(), right.data_ptr(), offs.data_ptr(),
              items.data_ptr(), items.shape[0], n_nodes, member.data_ptr(), member.shape[0], member.shape[1], floor.contiguous().data_ptr(),
              D, float(min_occ), best_q.data_ptr(), best_gain.data_ptr(), gains.data_ptr() if full else None,
              n_yes.data_ptr() if full else None, Q, ops._stream())
    return (best_q, best_gain, gains, n_yes) if full else (best_q, best_gain)


def tree_build(keys, roots, n_roots, fixed, member, gains_of, min_gain=0.0):
    """The full tree of the module docstring, level by level.  keys (N, 4): the items' (p, s, l, r); roots (N,): the root p S + s of
    every item; `fixed`: the roots that are leaves from the start; `gains_of([item index arrays])` -> (best question, its gain) per
    node, one call per level -> dict(question, yes, no, gain, root: lists over the nodes, -1 / -inf where a node does not split;
    items: the ascending item indices of every node)."""
    keys, roots, n_sets = np.asarray(keys), np.asarray(roots), member.shape[0]
    items = [np.nonzero(roots == m)[0] for m in range(n_roots)]
    t = {"question": [-1] * n_roots, "yes": [-1] * n_roots, "no": [-1] * n_roots, "gain": [-np.inf] * n_roots,
         "root": list(range(n_roots)), "items": items}
    fixed = set(int(m) for m in fixed)
    level = [m for m in range(n_roots) if m not in fixed and len(items[m])]
    while level:
        best_q, best_gain = gains_of([items[m] for m in level])
        nxt = []
        for m, q, g in zip(level, best_q, best_gain):
            q, g = int(q), float(g)
            if q < 0 or not g > min_gain:
                continue
            side = int(q >= n_sets)
            ans = member[q - side * n_sets, keys[items[m], 3 if side else 2]] != 0
            y = len(t["question"])
            for it in (items[m][ans], items[m][~ans]):
                t["question"].append(-1), t["yes"].append(-1), t["no"].append(-1), t["gain"].append(-np.inf)
                t["root"].append(t["root"][m]), items.append(it)
            t["question"][m], t["yes"][m], t["no"][m], t["gain"][m] = q, y, y + 1, g
            nxt += [y, y + 1]
        level = nxt
    return t


def check_leaves(budget, n_roots):
    """The leaf budget `triphones` against the roots of the tree, one per monophone state (fixed leaves included)."""
    if budget < n_roots:
        raise ValueError(f"triphones = {budget} leaves is below the {n_roots} roots and fixed leaves")


def tree_replay(tree, n_roots, budget):
    """The leaf budget: the recorded splits replayed through a priority queue, the largest gain first, the lowest node number on ties,
    until `budget` leaves exist or no split is left -> (question, yes, no, leaf: int32 arrays over the nodes of the full tree, -1
    where a node was not split / is no leaf of the pruned tree; the total gain of the splits kept)."""
    import heapq
    check_leaves(budget, n_roots)
    n = len(tree["question"])
    heap = [(-tree["gain"][m], m) for m in range(n_roots) if tree["question"][m] >= 0]
    heapq.heapify(heap)
    kept, live, leaves, total = np.zeros(n, bool), np.zeros(n, bool), n_roots, 0.0
    live[:n_roots] = True
    while heap and leaves < budget:
        g, m = heapq.heappop(heap)
        kept[m], leaves, total = True, leaves + 1, total - g
        for c in (tree["yes"][m], tree["no"][m]):
            live[c] = True
            if tree["question"][c] >= 0:
                heapq.heappush(heap, (-tree["gain"][c], c))
    question = np.where(kept, np.array(tree["question"]), -1).astype(np.int32)
    yes = np.where(kept, np.array(tree["yes"]), -1).astype(np.int32)
    no = np.where(kept, np.array(tree["no"]), -1).astype(np.int32)
    leaf = np.full(n, -1, np.int32)
    is_leaf = live & ~kept
    leaf[is_leaf] = np.arange(int(is_leaf.sum()), dtype=np.int32)
    return question, yes, no, leaf, total


def tree_leaves(question, yes, no, leaf, member, keys, states):
    """The leaf id of every logical state keys (N, 4) = (p, s, l, r), seen in training or not: from root p S + s down the tree."""
    keys = np.asarray(keys).reshape(-1, 4)
    node, n_sets = keys[:, 0].astype(np.int64) * states + keys[:, 1], member.shape[0]
    while True:
        q = question[node]
        go = q >= 0
        if not go.any():
            return leaf[node]
        side = q >= n_sets
        ans = member[np.where(go, q - side * n_sets, 0), np.where(side, keys[:, 3], keys[:, 2])] != 0
        node = np.where(go, np.where(ans, yes[node], no[node]), node)


def viterbi(E, lens, G, out=None, w=None, edge=None):
    """-> (backpointers uint8 like E, best end state (B,) int32, its score (B,) float64); under the arc costs w, edge when they are
    given, and the score then includes the end edge."""
    E, B, Tmax, _, lens_d = _check_scan(E, lens, G)
    arcs, costs = _arc_args(w, edge, B, G)
    bp = _out(out, E.shape, E.device, least=(), dtype=torch.uint8)
    end = torch.empty(B, dtype=torch.int32, device=E.device)
    score = torch.empty(B, dtype=torch.float64, device=E.device)
    _lib.call("fs2_align_viterbi" + arcs, E.data_ptr(), E.stride(0), E.stride(1), lens_d.data_ptr(), G.jlens.data_ptr(),
              G.skip.data_ptr(), G.ldg, G.alt.data_ptr(), *costs, bp.data_ptr(), bp.stride(0), bp.stride(1), end.data_ptr(),
              score.data_ptr(), B, Tmax, G.Jmax, ops._stream())
    return bp, end, score


def viterbi_arcs(E, lens, G, w, edge, out=None):
    """`viterbi` under the arc costs w (B, 3, >= Jmax) and edge (B, 4)."""
    return viterbi(E, lens, G, out, w, edge)


def backtrack(bp, lens, G, end):
    """-> frames per block (B, nbmax) int32 on the device."""
    bp = _dev(bp, torch.uint8, "bp")
    B, Tmax, Jmax = bp.shape
    if B != len(G.jl) or Jmax < G.Jmax:
        raise ValueError(f"bp {tuple(bp.shape)} does not hold {len(G.jl)} utterances of up to {G.Jmax} states")
    _, lens_d = ragged.lengths(lens, B, Tmax, "lens", bp.device)
    end = _dev(end, torch.int32, "end", 1)
    frames = torch.empty(B, max(G.nbmax, 1), dtype=torch.int32, device=bp.device)
    _lib.call("fs2_align_backtrack", bp.data_ptr(), bp.stride(0), bp.stride(1), lens_d.data_ptr(), G.jlens.data_ptr(),
              G.skip.data_ptr(), G.block.data_ptr(), G.ldg, end.data_ptr(), frames.data_ptr(), frames.shape[1], B, Tmax, G.Jmax,
              ops._stream())
    return frames


def path(bp, lens, G, end):
    """-> (state, cls): int32 (B, Tmax) on the device, the state of the Viterbi path at every frame and its emission class
    sid[state]; -1 in both at the frames a broken backpointer chain does not reach, nothing written at t >= T (the buffers start at
    -1)."""
    _no_host(bp=bp, end=end)
    bp = _dev(bp, torch.uint8, "bp")
    B, Tmax, Jmax = bp.shape
    if B != len(G.jl) or Jmax < G.Jmax:
        raise ValueError(f"bp {tuple(bp.shape)} does not hold {len(G.jl)} utterances of up to {G.Jmax} states")
    _, lens_d = ragged.lengths(lens, B, Tmax, "lens", bp.device)
    end = _dev(end, torch.int32, "end", 1)
    if end.shape[0] != B:
        raise ValueError(f"end holds {end.shape[0]} values for {B} utterances")
    both = torch.full((2, B, max(Tmax, 1)), -1, dtype=torch.int32, device=bp.device)
    state, cls = both[0], both[1]
    _lib.call("fs2_align_path", bp.data_ptr(), bp.stride(0), bp.stride(1), lens_d.data_ptr(), G.jlens.data_ptr(), G.skip.data_ptr(),
              G.sid.data_ptr(), G.ldg, end.data_ptr(), state.data_ptr(), state.stride(0), cls.data_ptr(), cls.stride(0), B, Tmax, G.Jmax,
              ops._stream())
    return state[:, :Tmax], cls[:, :Tmax]


def frame_scores(f, lens, cls, w, mu, var, out=None):
    """Every frame of f (B, Tmax, D) against every class of the mixture tables w (C, M), mu, var (C, M, D) (M = 1: w = 1) -> (own, best
    float64, arg int32), each (B, Tmax): the score of the frame's own class cls (B, >= Tmax) int32, the largest class score and the
    lowest class that attains it (the "Confidence" paragraph).  `out` = (own, best, arg) may be strided views of (B, >= Tmax); nothing
    at t >= T is written (fresh buffers hold NaN / -1 there)."""
    _no_host(f=f, cls=cls, w=w, mu=mu, var=var)
    f = _dev(f, torch.float64, "f")
    B, Tmax, D = f.shape
    if D == 0:
        raise ValueError("f has no feature dimension")
    w, mu, var, M = _check_mix(w, mu, var, D)
    C = w.shape[0]
    cls = _dev(cls, torch.int32, "cls", 2)
    if cls.shape[0] != B or cls.shape[1] < Tmax:
        raise ValueError(f"cls {tuple(cls.shape)} does not cover f {tuple(f.shape)}")
    _, lens_d = ragged.lengths(lens, B, Tmax, "lens", f.device)
    if out is None:
        own = torch.full((B, max(Tmax, 1)), float("nan"), dtype=torch.float64, device=f.device)
        best = torch.full_like(own, float("nan"))
        arg = torch.full((B, max(Tmax, 1)), -1, dtype=torch.int32, device=f.device)
    else:
        own, best, arg = out
        _no_host(own=own, best=best, arg=arg)
        own, best, arg = _dev(own, torch.float64, "own", 2), _dev(best, torch.float64, "best", 2), _dev(arg, torch.int32, "arg", 2)
        if any(t.shape[0] != B or t.shape[1] < Tmax for t in (own, best, arg)):
            raise ValueError(f"own, best and arg must be ({B}, >= {Tmax})")
    n_ws = _lib.load().fs2_align_frame_scores_ws(C, M, D)
    if n_ws == 0:
        raise ValueError(f"tables of {C} classes, {M} components and {D} dimensions exceed the supported size")
    ws = torch.empty(n_ws, dtype=torch.float64, device=f.device)
    _lib.call("fs2_align_frame_scores", f.data_ptr(), f.stride(0), f.stride(1), lens_d.data_ptr(), cls.data_ptr(), cls.stride(0),
              w.data_ptr(), mu.data_ptr(), var.data_ptr(), C, M, D, ws.data_ptr(), n_ws, own.data_ptr(), own.stride(0), best.data_ptr(),
              best.stride(0), arg.data_ptr(), arg.stride(0), B, Tmax, ops._stream())
    return own[:, :Tmax], best[:, :Tmax], arg[:, :Tmax]


def _ascending_sum(v):
    """the sum of v in index order (numpy's `sum` adds pairwise)"""
    return float(np.cumsum(v)[-1]) if len(v) else 0.0


def utterance_scores(graph, state, cls, own, best, arg, class_phone, viterbi):
    """The block and utterance numbers of the "Confidence" paragraph for one utterance from its per-frame arrays (T,): the path's
    state and class, own, best, arg; `viterbi` is the path's total score.  -> dict(frames, viterbi, loglik, gop, match, blocks
    (n_blocks, 3) = (loglik, gop, match) per block, NaN for a block of 0 frames)."""
    T = len(state)
    blk = np.asarray(graph["block"])[state]
    diff = own - best
    hit = (class_phone[arg] == class_phone[cls]).astype(np.float64)
    blocks = np.full((len(graph["blocks"]), 3), np.nan)
    edges = np.concatenate([[0], np.nonzero(blk[1:] != blk[:-1])[0] + 1, [T]])
    for a, b in zip(edges[:-1], edges[1:]):
        n = float(b - a)
        blocks[blk[a]] = (_ascending_sum(own[a:b]) / n, _ascending_sum(diff[a:b]) / n, _ascending_sum(hit[a:b]) / n)
    mand = ~np.array([bl[2] for bl in graph["blocks"]])[blk]
    n = float(mand.sum())
    return {"frames": T, "scored_frames": int(n), "viterbi": float(viterbi) / T, "loglik": _ascending_sum(own) / T,
            "gop": _ascending_sum(diff[mand]) / n, "match": _ascending_sum(hit[mand]) / n, "blocks": blocks}


def scores_summary(path, lowest=10):
    """The summary of a scores file `build(..., scores=path)` wrote: the corpus mean of `gop` over the frames of all mandatory blocks
    and the `lowest` utterances of lowest `gop`.  It reports; it sets no threshold."""
    with open(path, encoding="utf-8") as f:
        rows = [json.loads(line) for line in f if line.strip()]
    if not rows:
        return "scores: no utterances"
    n = [r["scored_frames"] for r in rows]
    gop, match = (sum(r[k] * m for r, m in zip(rows, n)) / sum(n) for k in ("gop", "match"))
    worst = sorted(rows, key=lambda r: (r["gop"], r["speaker"], r["basename"]))[:lowest]
    text = (f"scores: {len(rows)} utterances, mean gop {gop:.4f}, mean match {match:.4f} over {sum(n)} frames; lowest gop: " +
            ", ".join(f"{r['speaker']}/{r['basename']} {r['gop']:.4f}" for r in worst))
    if all("gop_seg" in r for r in rows):                                  # written with `seg_scores`
        seg = sum(r["gop_seg"] * m for r, m in zip(rows, n)) / sum(n)
        pairs = {}
        for r in rows:
            for p in r["phones"]:
                if p[8] is not None and p[7] is not None and p[8] < 0:
                    pairs[p[0], p[7]] = pairs.get((p[0], p[7]), 0) + 1
        top = sorted(pairs.items(), key=lambda kv: (-kv[1], kv[0]))[:20]
        text += (f"; mean gop_seg {seg:.4f}; intervals that lose to a rival: {sum(pairs.values())}" +
                 ("; most frequent: " + ", ".join(f"{p} -> {q} {c}" for (p, q), c in top) if top else ""))
    return text


def max_seg_phones():
    return _lib.load().fs2_align_max_seg_phones()


def segment_scores(f, lens, seg, cand, w, mu, var, arc, out=None):
    """Every segment seg (B, Kmax, 2) int32 = (start, frames) of f (B, Tmax, D) as a whole HMM of every candidate phone: cand (B, Kmax,
    P, S) int32 holds the class of every state of every candidate, arc (C, 2) = (log stay, log leave) per class of the mixture
    tables w (C, M), mu, var (C, M, D) -> V (B, Kmax, P) float64 (the "Segmental scores" paragraph).  `out` may be a strided view of
    (B, Kmax, >= P); the row of an absent segment (frames <= 0, outside the utterance, a negative candidate) is not written (a
    fresh buffer holds NaN there).  A candidate class >= C is a ValueError before the launch."""
    _no_host(f=f, seg=seg, cand=cand, w=w, mu=mu, var=var, arc=arc)
    f = _dev(f, torch.float64, "f")
    B, Tmax, D = f.shape
    if D == 0:
        raise ValueError("f has no feature dimension")
    w, mu, var, M = _check_mix(w, mu, var, D)
    C = w.shape[0]
    seg, cand = _dev(seg, torch.int32, "seg").contiguous(), _dev(cand, torch.int32, "cand", 4).contiguous()
    Kmax, P, S = cand.shape[1:]
    if seg.shape != (B, Kmax, 2) or cand.shape[0] != B:
        raise ValueError(f"seg {tuple(seg.shape)} and cand {tuple(cand.shape)} do not describe the blocks of {B} utterances")
    if not 1 <= P <= max_seg_phones() or not 1 <= S <= 3:
        raise ValueError(f"{P} candidate phones of {S} states, supported are 1..{max_seg_phones()} phones of 1..3 states")
    arc = _dev(arc, torch.float64, "arc", 2).contiguous()
    if arc.shape != (C, 2):
        raise ValueError(f"arc {tuple(arc.shape)} is not ({C}, 2)")
    if cand.numel() and int(cand.max()) >= C:
        raise ValueError(f"cand holds class {int(cand.max())}, the tables have {C}")
    _, lens_d = ragged.lengths(lens, B, Tmax, "lens", f.device)
    if out is None:
        V = torch.full((B, max(Kmax, 1), P), float("nan"), dtype=torch.float64, device=f.device)
    else:
        _no_host(out=out)
        V = _dev(out, torch.float64, "out")
        if V.shape[0] != B or V.shape[1] < Kmax or V.shape[2] < P or (V.numel() and V.stride(0) < V.shape[1] * V.stride(1)):
            raise ValueError(f"out must be ({B}, >= {Kmax}, >= {P}), got {tuple(V.shape)}")
    n_ws = _lib.load().fs2_align_segment_scores_ws(C, M, D)
    if n_ws == 0:
        raise ValueError(f"tables of {C} classes, {M} components and {D} dimensions exceed the supported size")
    ws = torch.empty(n_ws, dtype=torch.float64, device=f.device)
    _lib.call("fs2_align_segment_scores", f.data_ptr(), f.stride(0), f.stride(1), lens_d.data_ptr(), seg.data_ptr(), seg.stride(0),
              cand.data_ptr(), cand.stride(0), cand.stride(1), w.data_ptr(), mu.data_ptr(), var.data_ptr(), C, M, D, arc.data_ptr(),
              ws.data_ptr(), n_ws, V.data_ptr(), V.stride(0), V.stride(1), B, Tmax, Kmax, P, S, ops._stream())
    return V[:, :Kmax, :P]


def segment_table(graph, state):
    """(n_blocks, 2) int32 = (start, frames) of every block on the per-frame path `state` (T,); a block the path skips is (0, 0)."""
    blk = np.asarray(graph["block"])[state]
    out = np.zeros((len(graph["blocks"]), 2), np.int32)
    edges = np.concatenate([[0], np.nonzero(blk[1:] != blk[:-1])[0] + 1, [len(blk)]])
    for a, b in zip(edges[:-1], edges[1:]):
        out[blk[a]] = (a, b - a)
    return out


def block_phones(graph):
    """The phone id of every block of a monophone graph (`utterance_graph`: state k S + s has class phone_id S + s)."""
    S = len(graph["sid"]) // len(graph["blocks"])
    return np.asarray(graph["sid"], np.int64)[::S] // S


def segment_reductions(graph, seg, V):
    """The block and utterance numbers of the "Segmental scores" paragraph for the monophone graph of one utterance from seg
    (n_blocks, 2) and V (n_blocks, P) -> (blocks (n_blocks, 3) = (gop_seg, rival, margin), NaN for a block of 0 frames; the
    utterance's gop_seg, the mean over the frames of the mandatory blocks in block order)."""
    out = np.full((len(graph["blocks"]), 3), np.nan)
    num, den, phones = 0.0, 0.0, block_phones(graph)
    for k, (_, _, optional) in enumerate(graph["blocks"]):
        n = int(seg[k, 1])
        if n == 0:
            continue
        if V.shape[1] == 1:
            out[k, 2] = 0.0
            continue
        p = int(phones[k])
        rest = V[k].copy()
        rest[p] = -np.inf
        rival = int(np.argmax(rest))                                       # the first of the largest
        if rival == p:                                                     # every rival at -inf: the lowest q != p
            rival = 1 if p == 0 else 0
        margin = (V[k, p] - V[k, rival]) / n
        out[k] = (min(margin, 0.0), rival, margin)
        if not optional:
            num, den = num + out[k, 0] * n, den + n
    return out, num / den if den else float("nan")


# ------------------------------------------------------------------------------------------------ the model
def fmllr_dim_message(dim, lda):
    return (f"fmllr adapts at most {max_fmllr_dim()} feature dimensions (a speaker's statistics are D (D + 1)(D + 2) doubles), got {dim}"
            + ("" if lda else f": with {dim // 2} mel channels --fmllr needs --lda k with k <= {max_fmllr_dim()}"))


def check_options(dim, mixtures=1, mix_iters=4, lda=0, splice=3, lda_iters=4, fmllr=0, fmllr_rounds=2, fmllr_iters=2, fmllr_sweeps=20,
                  fmllr_min_frames=500, triphones=0, tri_iters=4, tri_min_occ=100, tri_min_gain=0.0, transitions=0):
    """The stage switches of `Aligner` and `build` for features of `dim` = 2 n_mel columns; a bad one is a ValueError before any
    work -> (n_mel, D_s of the LDA or 0, the dimension the Gaussian stages after the LDA see)."""
    n_mel, Ds = dim // 2, 0
    if int(transitions) not in (0, 1):
        raise ValueError(f"transitions must be 0 or 1, got {transitions}")
    if int(lda) != 0:
        if dim % 2:
            raise ValueError(f"dim {dim} is not 2 n_mel")
        Ds = splice_dim(n_mel, int(splice), int(lda))
        if int(lda_iters) < 0:
            raise ValueError(f"lda_iters must not be negative, got {lda_iters}")
        dim = int(lda)
    if int(fmllr) != 0:
        if int(fmllr) != 1:
            raise ValueError(f"fmllr must be 0 or 1, got {fmllr}")
        if not 1 <= dim <= max_fmllr_dim():
            raise ValueError(fmllr_dim_message(dim, int(lda)))
        if int(fmllr_rounds) < 1 or int(fmllr_iters) < 0 or int(fmllr_sweeps) < 1 or float(fmllr_min_frames) < 0:
            raise ValueError(f"fmllr_rounds {fmllr_rounds} and fmllr_sweeps {fmllr_sweeps} must be at least 1, fmllr_iters "
                             f"{fmllr_iters} and fmllr_min_frames {fmllr_min_frames} not negative")
    if int(triphones) != 0:
        if not float(tri_min_occ) >= 1.0:
            raise ValueError(f"tri_min_occ must be at least 1, got {tri_min_occ}")
        if int(tri_iters) < 0 or not float(tri_min_gain) >= 0.0:
            raise ValueError(f"tri_iters {tri_iters} and tri_min_gain {tri_min_gain} must not be negative")
    if int(mixtures) != 1:
        if not 1 <= int(mixtures) <= max_mixtures():
            raise ValueError(f"mixtures must be 1..{max_mixtures()}, got {mixtures}")
        if int(mix_iters) < 1:
            raise ValueError(f"mix_iters must be at least 1, got {mix_iters}")
    return n_mel, Ds, dim


class Aligner:
    """The class table (mu, var: (n_classes, dim) float64) on the device, trained by `fit`, used by `align`.  With `mixtures` = M > 1
    `fit` goes on from that table to the mixture tables gw (n_classes, M), gmu, gvar (n_classes, M, dim) on the device and ncomp
    (active components per class, numpy), and `align` decodes with those.  With `lda` = k > 0 `fit` goes on from the table in x to
    the transform P (k, D_s), o (k,) and to tables of k columns (mu, var and the mixture tables), and `align` decodes in z.  With
    `fmllr` = 1 `fit` goes on to the speaker transforms W (n_spk, D, D + 1) and to tables trained on the adapted features, and
    `fit` and `align` take the speaker index of every utterance.  With `triphones` = L > 0 (and `phone_ids`, the phone table) `fit`
    goes on from the last single-Gaussian table to the decision tree `tree` (arrays over its nodes) and to tables over its leaves,
    `n_classes` becomes the leaf count and `align` decodes on the leaves.  With `transitions` = 1 every Baum-Welch pass also trains
    loop (n_classes,) and opt (3,) (numpy float64: the self-loop probability of every class, the probability that an optional block
    of kind 0 / 1 / 2 is taken), every pass runs under their arc costs and `align` decodes with them."""

    def __init__(self, n_classes, dim, states=2, device="cuda", mixtures=1, mix_iters=4, min_split_occ=40, lda=0, splice=3, lda_iters=4,
                 fmllr=0, fmllr_rounds=2, fmllr_iters=2, fmllr_sweeps=20, fmllr_min_frames=500, triphones=0, tri_iters=4, tri_min_occ=100,
                 tri_min_gain=0.0, questions=None, phone_ids=None, transitions=0):
        self.device = ragged.require_device(torch.device(device), "fastspeech2_amd.align")
        if n_classes % states:
            raise ValueError(f"n_classes {n_classes} is not a multiple of states {states}")
        self.n_classes, self.n_mono, self.dim, self.states = n_classes, n_classes, dim, states
        self.mu = torch.zeros(n_classes, dim, dtype=torch.float64, device=self.device)
        self.var = torch.ones(n_classes, dim, dtype=torch.float64, device=self.device)
        self.floor = np.zeros(dim)
        self.n_mel, self.splice_dim, dim = check_options(                  # the tables after the LDA live in z: dim = lda
            dim, mixtures, mix_iters, lda, splice, lda_iters, fmllr, fmllr_rounds, fmllr_iters, fmllr_sweeps, fmllr_min_frames, triphones,
            tri_iters, tri_min_occ, tri_min_gain, transitions)
        self.transitions = int(transitions)
        self.loop, self.opt = np.full(n_classes, 0.5), np.full(3, 0.5)
        self.mixtures, self.mix_iters, self.min_split_occ = int(mixtures), int(mix_iters), float(min_split_occ)
        self.lda, self.splice, self.lda_iters, self.P, self.o = int(lda), int(splice), int(lda_iters), None, None
        self.fmllr, self.W, self.n_spk = int(fmllr), None, 0
        self.fmllr_rounds, self.fmllr_iters, self.fmllr_sweeps = int(fmllr_rounds), int(fmllr_iters), int(fmllr_sweeps)
        self.fmllr_min_frames = float(fmllr_min_frames)
        self.triphones, self.tri_iters, self.tri_min_occ, self.tri_min_gain = int(triphones), int(tri_iters), float(tri_min_occ), float(tri_min_gain)
        self.questions, self.phone_ids, self.tree = questions, phone_ids, None
        if self.triphones != 0:
            if phone_ids is None or len(phone_ids) * states != n_classes or any(p not in phone_ids for p in (SIL, SP, SPN)):
                raise ValueError(f"an Aligner with triphones needs `phone_ids`, the phone table of its {n_classes // states} phones")
            check_leaves(triphones, n_classes)
            self.question_sets = read_questions(questions, phone_ids) if questions is not None else None
            if self.question_sets is not None and len(self.question_sets[0]) > max_tree_sets():
                raise ValueError(f"{len(self.question_sets[0])} question sets, supported are 1..{max_tree_sets()}")
        if self.mixtures != 1:
            self._mixture_tables(n_classes, dim)

    def _mixture_tables(self, C, dim):
        """Fresh mixture tables for C classes: every class one active component of weight 1."""
        self.gw = torch.zeros(C, self.mixtures, dtype=torch.float64, device=self.device)
        self.gw[:, 0] = 1.0
        self.gmu = torch.zeros(C, self.mixtures, dim, dtype=torch.float64, device=self.device)
        self.gvar = torch.ones(C, self.mixtures, dim, dtype=torch.float64, device=self.device)
        self.ncomp = np.ones(C, np.int64)

    def _prepare(self, feats, lens, graphs):
        lens = [int(v) for v in lens]
        if len(lens) != len(graphs) or len(lens) != feats.shape[0]:
            raise ValueError(f"{feats.shape[0]} feature rows, {len(lens)} lengths and {len(graphs)} graphs")
        if feats.dim() != 3 or feats.shape[2] != self.dim or feats.dtype != torch.float64:
            raise ValueError(f"feats must be (B, Tmax, {self.dim}) float64, got {feats.dtype} {tuple(feats.shape)}")
        for n, g in zip(lens, graphs):
            if n < g["mandatory"] or n > feats.shape[1]:
                raise ValueError(f"an utterance of {n} frames cannot pass its {g['mandatory']} mandatory states "
                                 f"(or exceeds the {feats.shape[1]} rows of feats)")
        G = Graphs(graphs, self.device)
        return lens, G

    def _set(self, mu, var):
        if tuple(self.mu.shape) != mu.shape:                               # between the table in x and the table in z
            self.mu = torch.empty(mu.shape, dtype=torch.float64, device=self.device)
            self.var = torch.empty(mu.shape, dtype=torch.float64, device=self.device)
        self.mu.copy_(torch.from_numpy(np.ascontiguousarray(mu)))
        self.var.copy_(torch.from_numpy(np.ascontiguousarray(var)))

    def _speakers(self, speakers, B, n_spk=None):
        """The speaker indices of one batch, checked (None without fmllr)."""
        if not self.fmllr:
            return None
        if speakers is None:
            raise ValueError("an Aligner with fmllr needs the speaker index of every utterance (`speakers`)")
        return _speaker_list(speakers, B, n_spk if n_spk is not None else np.iinfo(np.int32).max)

    def _arcs(self, prep):
        """The device arc costs of every batch, rebuilt from the tables (nothing without transitions)."""
        if self.transitions:
            for _, _, G, _ in prep:
                G.set_arcs(self.loop, self.opt)

    def _tacc(self):
        """The accumulators of one pass's arc posteriors: [class sums (C, 5), sums per kind of optional block (6, 5)]."""
        return [None, None] if self.transitions else None

    def _fb(self, E, lens, G, tacc=None):
        """gamma and the log-likelihoods of one batch from its emissions: forward and backward, with transitions under the current
        arc costs, the sums of the arc posteriors added to `tacc`."""
        if not self.transitions:
            alpha, loglik = forward(E, lens, G)
            return backward(E, lens, G, alpha, loglik), loglik
        alpha, loglik = forward(E, lens, G, w=G.w, edge=G.edge)
        gamma, xi = backward(E, lens, G, alpha, loglik, w=G.w, edge=G.edge)
        if tacc is not None:
            classes, kinds = G.arc_index(self.n_classes)
            tacc[0] = reduce(xi, G, self.n_classes, tacc[0], classes)
            tacc[1] = reduce(xi, G, 6, tacc[1], kinds)
        return gamma, loglik

    def _e_step(self, prep, each, tacc=None, mixtures=False):
        """The E-step of one pass over `prep` = [(features, lens, Graphs, index)].  Per batch: the features to the device, the
        emissions (from the single-Gaussian table, or with `mixtures` from the mixture tables, with their responsibilities),
        forward and backward under the current arc costs with the arc posteriors added to `tacc`, then `each(batch number, x, lens,
        G, index, gamma, resp)` takes from the posteriors what the pass needs.  `batches_by_bytes` budgets for the buffers of one
        batch: they are released before the next batch's are allocated, and `each` must keep no reference to gamma or resp.
        -> the sum of all utterances' log-likelihoods, added batch after batch."""
        total = 0.0
        for i, (feats, lens, G, index) in enumerate(prep):
            x = feats.to(self.device, non_blocking=True)
            if mixtures:
                resp = torch.empty(x.shape[0], x.shape[1], G.ldg, self.mixtures, dtype=torch.float64, device=self.device)
                E = emit_gmm(x, lens, G, self.gw, self.gmu, self.gvar, resp=resp)
            else:
                resp, E = None, emit(x, lens, G, self.mu, self.var)
            gamma, loglik = self._fb(E, lens, G, tacc)
            del E
            each(i, x, lens, G, index, gamma, resp)
            total += float(np.sum(loglik.cpu().numpy()))
            del x, gamma, resp
        return total

    def _pass(self, prep, mu, var, n_frames, jac=0.0):
        """One Baum-Welch pass of the single-Gaussian table over `prep`: the class sums, then the update of (mu, var) and of the
        transition tables -> (the class sums, mu, var, the value the pass reports: (log-likelihood + `jac`) / n_frames, `jac` the
        fMLLR Jacobian term)."""
        sums, tacc = None, self._tacc()

        def each(i, x, lens, G, index, gamma, resp):
            nonlocal sums
            sums = reduce(stats(gamma, x, lens, G), G, self.n_classes, sums, index)
        total = self._e_step(prep, each, tacc)
        s = sums.cpu().numpy()
        mu, var = m_step(s, mu, var, self.floor)
        self._set(mu, var)
        self._trans_step(s[:, 0], tacc, prep)
        return s, mu, var, (total + jac) / n_frames

    def _initial_tables(self, s):
        """The first table of a feature space from its first class sums s: the global mean g and variance v of their total, the
        floor 1e-2 v, every class at (g, v), then the update -> (mu, var)."""
        C, dim = s.shape[0], (s.shape[1] - 1) // 2
        tot = s.sum(axis=0)
        g_mean = tot[1:1 + dim] / tot[0]
        g_var = tot[1 + dim:] / tot[0] - g_mean * g_mean
        self.floor = VAR_FLOOR * g_var
        mu, var = m_step(s, np.tile(g_mean, (C, 1)), np.tile(g_var, (C, 1)), self.floor)
        self._set(mu, var)
        return mu, var

    def _trans_step(self, n, tacc, prep):
        """The transition update after a pass with the class occupancies n, and the new arc costs on every batch of `prep`."""
        if not self.transitions:
            return
        c, o = tacc[0].cpu().numpy(), tacc[1].cpu().numpy()
        self.loop, self.opt = trans_step(n, c[:, 0], o[[0, 2, 4], [3, 1, 1]], o[[1, 3, 5], [3, 2, 4]], self.loop, self.opt)
        self._arcs(prep)

    def _trans_log(self, stage):
        if self.transitions:
            d = 1.0 / (1.0 - self.loop)
            print(f"transitions: {stage}, opt " + " ".join(f"{v:.4f}" for v in self.opt) + f", frames per state {d.min():.4g} .. {d.max():.4g}")

    def fit(self, batches, iters=12, speakers=None):
        """batches: [(feats (B, Tmax, D) float64 on the device or the host, lens, graphs)].  Flat start, then `iters` Baum-Welch
        passes (then, with lda, fmllr and mixtures, their stages); returns the log-likelihood per frame of every pass.  `speakers`
        (with fmllr): one list of speaker indices per batch."""
        batches = list(batches)
        self.n_classes, self.tree = self.n_mono, None                      # the stages before the tree train the monophones
        if self.fmllr:
            if speakers is None or len(speakers) != len(batches):
                raise ValueError("an Aligner with fmllr needs one list of speaker indices per batch (`speakers`)")
            speakers = [self._speakers(sp, b[0].shape[0]) for sp, b in zip(speakers, batches)]
        prep = []
        for feats, lens, graphs in batches:
            lens, G = self._prepare(feats, lens, graphs)
            prep.append((feats, lens, G, G.index(self.n_classes, G.ldg)))
        n_frames = sum(sum(lens) for _, lens, _, _ in prep)
        self.loop, self.opt = np.full(self.n_classes, 0.5), np.full(3, 0.5)
        self._arcs(prep)

        # flat start: the hard assignment as a one-hot gamma through the same statistics kernels
        sums = None
        for feats, lens, G, index in prep:
            x = feats.to(self.device, non_blocking=True)
            B, Tmax = x.shape[0], x.shape[1]
            assign = np.zeros((B, Tmax), np.int64)
            for b, g in enumerate(G.graphs):
                assign[b, :lens[b]] = flat_assignment(g, lens[b])
            gamma = torch.zeros(B, Tmax, G.ldg, dtype=torch.float64, device=self.device)
            gamma.scatter_(2, _up(assign, self.device).unsqueeze(2), 1.0)
            sums = reduce(stats(gamma, x, lens, G), G, self.n_classes, sums, index)
            del gamma
        if sums is None:
            raise ValueError("no utterances to train on")
        s = sums.cpu().numpy()
        mu, var = self._initial_tables(s)

        history = []
        for _ in range(iters):
            s, mu, var, ll = self._pass(prep, mu, var, n_frames)
            history.append(ll)
        self._trans_log("monophones")
        if self.lda:
            prep, s, mu, var, more = self._fit_lda(prep, n_frames)
            history += more
        jac = 0.0
        if self.fmllr:
            prep, s, mu, var, more, jac = self._fit_fmllr(prep, speakers, n_frames, s, mu, var)
            history += more
        if self.triphones:
            prep, s, mu, var, more = self._fit_triphones(prep, n_frames, mu, var, jac)
            history += more
        if self.mixtures > 1:
            history += self._fit_mixtures(prep, n_frames, s[:, 0], mu, var, jac)
        return history

    def _project(self, x, lens):
        return project(splice(x, lens, self.n_mel, self.splice), lens, self.P, self.o)

    def _fit_lda(self, prep, n_frames):
        """Steps 2 to 5 of the LDA schedule from the table in x -> (prep with z for the features, the class sums of the last pass,
        mu, var in z, the log-likelihood per frame of the statistics pass and of the passes in z)."""
        C, Ds, k = self.n_classes, self.splice_dim, self.lda
        sums, sv, sm, zprep = None, None, None, []

        def spliced(i, x, lens, G, index, gamma, resp):                    # the statistics pass
            nonlocal sums, sv, sm
            y = splice(x, lens, self.n_mel, self.splice)
            sums = reduce(stats(gamma, y, lens, G), G, C, sums, index)
            sv, sm = scatter(y, lens, sv, sm)
        history = [self._e_step(prep, spliced) / n_frames]
        cs = sums.cpu().numpy()
        P, o, eig = lda_transform(cs[:, 0], cs[:, 1:1 + Ds], float(n_frames), sv.cpu().numpy(), sm.cpu().numpy(), k)
        print("lda: eigenvalues " + " ".join(f"{v:.4g}" for v in eig))
        self.P, self.o = _up(P, self.device), _up(o, self.device)

        def projected(i, x, lens, G, index, gamma, resp):                  # the same gamma on z
            nonlocal sums
            z = self._project(x, lens)
            sums = reduce(stats(gamma, z, lens, G), G, C, sums, index)
            zprep.append((z.to(prep[i][0].device), lens, G, index))
        sums = None                                                        # the statistics pass's sums on y are spent
        self._e_step(prep, projected)
        s = sums.cpu().numpy()
        mu, var = self._initial_tables(s)
        for _ in range(self.lda_iters):
            s, mu, var, ll = self._pass(zprep, mu, var, n_frames)
            history.append(ll)
        self._trans_log("lda")
        return zprep, s, mu, var, history

    def _fit_fmllr(self, prep, speakers, n_frames, s, mu, var):
        """The fMLLR rounds from the single-Gaussian table (mu, var) on the features of `prep` -> (prep with the adapted features,
        the class sums of the last pass, mu, var, the reported value of every pass, sum_u T_u log|det A_s(u)| of the final W)."""
        D = mu.shape[1]
        S = self.n_spk = 1 + max((int(sp.max()) for sp in speakers if sp.size), default=0)
        W = np.tile(np.eye(D, D + 1), (S, 1, 1))
        self.W = _up(W, self.device)
        spk_frames = np.zeros(S)
        for (_, lens, _, _), sp in zip(prep, speakers):
            np.add.at(spk_frames, sp, np.asarray(lens, np.float64))

        def adapted():
            return [(fmllr_apply(feats.to(self.device, non_blocking=True), lens, self.W, sp).to(feats.device), lens, G, index)
                    for (feats, lens, G, index), sp in zip(prep, speakers)]
        hprep, history, jac, acc = adapted(), [], 0.0, None

        def accumulate(i, fh, lens, G, index, gamma, resp):                # the statistics pass: (beta, G, k) on the unadapted features
            nonlocal acc
            c, h = fmllr_weights(gamma, lens, G, self.mu, self.var)
            acc = fmllr_accumulate(prep[i][0].to(self.device, non_blocking=True), c, h, lens, speakers[i], S, *acc)
        for rnd in range(self.fmllr_rounds):
            acc = (None, None, None)
            history.append((self._e_step(hprep, accumulate) + jac) / n_frames)
            W, status = fmllr_update(*(t.cpu().numpy() for t in acc), W, self.fmllr_min_frames, self.fmllr_sweeps)
            acc = None
            logdet = np.linalg.slogdet(W[:, :, :D])[1]
            jac = float(np.dot(spk_frames, logdet))
            print(f"fmllr: round {rnd + 1}, {int(np.sum(status == 0))} speakers adapted, {int(np.sum(status == 1))} kept (too few "
                  f"frames), {int(np.sum(status == 2))} kept (not positive definite), mean log|det A| {float(np.mean(logdet)):.4g}")
            self.W.copy_(torch.from_numpy(np.ascontiguousarray(W)))
            hprep = adapted()
            for _ in range(self.fmllr_iters):
                s, mu, var, ll = self._pass(hprep, mu, var, n_frames, jac)
                history.append(ll)
        self._trans_log("fmllr")
        return hprep, s, mu, var, history, jac

    def _leaf_graph(self, graph):
        """The graph with `sid` = the leaf of every state's logical state (the topology is untouched)."""
        t = self.tree
        ctx = triphone_contexts(graph, self.phone_ids, self.states)
        sid = tree_leaves(t["question"], t["yes"], t["no"], t["leaf"], t["member"], ctx[:, [1, 3, 0, 2]], self.states)
        return dict(graph, sid=sid.astype(np.int32))

    def _fit_triphones(self, prep, n_frames, mu, var, jac=0.0):
        """The triphone stage from the single-Gaussian monophone table (mu, var) on the features of `prep` -> (prep with the leaf
        graphs, the leaf sums of the last pass, mu, var over the leaves, the reported value of the statistics pass and of the
        `tri_iters` passes).  `jac` (fmllr) is added to every pass's total log-likelihood."""
        S, C0, D = self.states, self.n_classes, mu.shape[1]
        n_sym, cols = len(self.phone_ids) + 1, 1 + 2 * mu.shape[1]
        code = lambda k: ((k[:, 0].astype(np.int64) * S + k[:, 1]) * n_sym + k[:, 2]) * n_sym + k[:, 3]     # noqa: E731
        ctxs = [[triphone_contexts(g, self.phone_ids, S)[:, [1, 3, 0, 2]] for g in G.graphs] for _, _, G, _ in prep]
        keys = np.unique(np.concatenate([k for b in ctxs for k in b]), axis=0)       # the items, sorted by (p, s, l, r)
        codes, n_items = code(keys), len(keys)

        sums = None

        def by_item(i, x, lens, G, index, gamma, resp):                    # the statistics pass over the items
            nonlocal sums
            Gi = Graphs([dict(g, sid=np.searchsorted(codes, code(k)).astype(np.int32)) for g, k in zip(G.graphs, ctxs[i])], self.device)
            sums = reduce(stats(gamma, x, lens, G), Gi, n_items, sums, Gi.index(n_items, G.ldg))
        history = [(self._e_step(prep, by_item) + jac) / n_frames]

        def pooled(classes, n):                                            # class sums of the item table, items ascending
            return reduce(sums.view(1, n_items, cols), None, n, None, _csr(classes, n, self.device)).cpu().numpy()
        roots = keys[:, 0].astype(np.int64) * S + keys[:, 1]
        ci = sorted(self.phone_ids[p] for p in (SIL, SP, SPN))
        if self.question_sets is not None:
            names, member = self.question_sets
        else:
            names, member = phone_questions(pooled(roots, C0), [p for p in range(C0 // S) if p not in ci], S, self.floor, n_sym)
        if not 1 <= len(names) <= max_tree_sets():
            raise ValueError(f"{len(names)} question sets, supported are 1..{max_tree_sets()}")
        left, right = _up(keys[:, 2].astype(np.int32), self.device), _up(keys[:, 3].astype(np.int32), self.device)
        member_d, floor_d = _up(member, self.device), _up(self.floor, self.device)

        def gains_of(nodes):                                               # one launch per level
            offs, items = _csr(np.repeat(np.arange(len(nodes)), [len(it) for it in nodes]), len(nodes), self.device, np.concatenate(nodes))
            q, g = tree_gains(sums, left, right, offs, items, member_d, floor_d, self.tri_min_occ)
            return q.cpu().numpy(), g.cpu().numpy()
        full = tree_build(keys, roots, C0, [p * S + st for p in ci for st in range(S)], member, gains_of, self.tri_min_gain)
        question, yes, no, leaf, gain = tree_replay(full, C0, self.triphones)
        n_leaves = int(leaf.max()) + 1
        self.tree = {"question": question, "yes": yes, "no": no, "leaf": leaf, "member": member, "names": names, "gain": gain,
                     "n_items": n_items, "n_leaves": n_leaves}
        print(f"triphones: {n_items} items, {2 * len(names)} questions, {n_leaves} leaves, total gain {gain:.6g}")

        item_leaf = tree_leaves(question, yes, no, leaf, member, keys, S)
        leaf_root = np.zeros(n_leaves, np.int64)
        leaf_root[leaf[leaf >= 0]] = np.array(full["root"])[leaf >= 0]
        s = pooled(item_leaf.astype(np.int64), n_leaves)
        mu, var = m_step(s, mu[leaf_root], var[leaf_root], self.floor)
        del sums
        self.n_classes = n_leaves
        self._set(mu, var)
        self.loop = self.loop[leaf_root]                                   # a leaf starts from its root's self-loop probability
        if self.mixtures > 1:
            self._mixture_tables(n_leaves, D)
        lprep = []
        for (feats, lens, G, _), kb in zip(prep, ctxs):
            Gl = Graphs([dict(g, sid=item_leaf[np.searchsorted(codes, code(k))].astype(np.int32)) for g, k in zip(G.graphs, kb)], self.device)
            lprep.append((feats, lens, Gl, Gl.index(n_leaves, Gl.ldg)))
        self._arcs(lprep)
        for _ in range(self.tri_iters):
            s, mu, var, ll = self._pass(lprep, mu, var, n_frames, jac)
            history.append(ll)
        self._trans_log("triphones")
        return lprep, s, mu, var, history

    def _fit_mixtures(self, prep, n_frames, occ0, mu, var, jac=0.0):
        """The split stages k = 1 .. M - 1 from the one-component table (mu, var) whose last pass had the occupancies occ0; `jac`
        (fmllr) is added to every pass's total log-likelihood."""
        C, M, D = self.n_classes, self.mixtures, mu.shape[1]
        w, gmu, gvar = np.zeros((C, M)), np.zeros((C, M, D)), np.ones((C, M, D))
        w[:, 0], gmu[:, 0], gvar[:, 0] = 1.0, mu, var
        ncomp, occ = np.ones(C, np.int64), np.zeros((C, M))
        occ[:, 0] = occ0
        mprep = [(feats, lens, G, G.index(C, G.ldg, M)) for feats, lens, G, _ in prep]
        history, sums = [], None

        def each(i, x, lens, G, index, gamma, resp):
            nonlocal sums
            sums = reduce(stats_gmm(gamma, resp, x, lens, G), G, C, sums, index)

        def set_tables():
            for dst, src in ((self.gw, w), (self.gmu, gmu), (self.gvar, gvar)):
                dst.copy_(torch.from_numpy(np.ascontiguousarray(src)))
        for k in range(1, M):
            w, gmu, gvar, ncomp = split_classes(w, gmu, gvar, ncomp, occ, k, self.min_split_occ)
            print(f"mixtures: stage {k + 1}, classes by active components " +
                  " ".join(f"{n}:{int(np.sum(ncomp == n))}" for n in range(1, M + 1) if np.any(ncomp == n)))
            for _ in range(self.mix_iters):
                set_tables()
                sums, tacc = None, self._tacc()
                total = self._e_step(mprep, each, tacc, mixtures=True)
                s = sums.cpu().numpy().reshape(C, M, 1 + 2 * D)
                occ = s[:, :, 0]
                w, gmu, gvar = m_step_gmm(s, w, gmu, gvar, ncomp, self.floor)
                if self.transitions:
                    n_c = np.zeros(C)
                    for m in range(M):                                     # the class occupancy: the active components, ascending
                        n_c = n_c + np.where(m < ncomp, occ[:, m], 0.0)
                    self._trans_step(n_c, tacc, prep)
                history.append((total + jac) / n_frames)
            self._trans_log(f"mixtures stage {k + 1}")
        set_tables()
        self.ncomp = ncomp
        return history

    def _decode(self, feats, lens, graphs, speakers):
        """The feature pipeline and the Viterbi pass `align` and `score` share -> (the features the decoding model sees, lens, the
        batch's Graphs, backpointers, end states, Viterbi scores)."""
        if self.fmllr and self.W is None:
            raise ValueError("an Aligner with fmllr has no transforms before `fit`")
        speakers = self._speakers(speakers, feats.shape[0], self.n_spk)
        if self.triphones:
            if self.tree is None:
                raise ValueError("an Aligner with triphones has no tree before `fit`")
            graphs = [self._leaf_graph(g) for g in graphs]
        lens, G = self._prepare(feats, lens, graphs)
        x = feats.to(self.device, non_blocking=True)
        if self.lda:
            if self.P is None:
                raise ValueError("an Aligner with lda has no transform before `fit`")
            x = self._project(x, lens)
        if self.fmllr:
            x = fmllr_apply(x, lens, self.W, speakers)
        E = emit(x, lens, G, self.mu, self.var) if self.mixtures == 1 else emit_gmm(x, lens, G, self.gw, self.gmu, self.gvar)
        if self.transitions:
            G.set_arcs(self.loop, self.opt)
        bp, end, vit = viterbi(E, lens, G, w=G.w, edge=G.edge)             # no costs (None) without transitions
        return x, lens, G, bp, end, vit

    def align(self, feats, lens, graphs, speakers=None):
        """Viterbi alignment of one ragged batch -> [frames per block (int32 numpy)] per utterance.  `speakers` (with fmllr): the
        speaker index of every row."""
        _, lens, G, bp, end, _ = self._decode(feats, lens, graphs, speakers)
        frames = backtrack(bp, lens, G, end).cpu().numpy()
        return [frames[b, :len(g["blocks"])].copy() for b, g in enumerate(graphs)]

    def class_phone(self):
        """(n_classes,) int64: the phone of every emission class at decode time: c // states for monophone states, the phone of the
        leaf's root after `triphones` (built from `tree`)."""
        if not self.triphones:
            return np.arange(self.n_classes, dtype=np.int64) // self.states
        if self.tree is None:
            raise ValueError("an Aligner with triphones has no tree before `fit`")
        t = self.tree
        out = np.full(t["n_leaves"], -1, np.int64)
        for root in range(self.n_mono):                                    # the roots are the nodes p S + s
            todo = [root]
            while todo:
                node = todo.pop()
                if t["leaf"][node] >= 0:
                    out[t["leaf"][node]] = root // self.states
                else:
                    todo += [int(t["yes"][node]), int(t["no"][node])]
        return out

    def candidates(self, graph):
        """(n_blocks, P S) int32: the candidate classes of the "Segmental scores" paragraph for the monophone graph of one utterance:
        q S + s, or after `triphones` the leaf of (l_k, q, r_k, s), the block's own contexts (`#` on both sides when the block's
        phone or q is context-independent)."""
        S, P, K = self.states, self.n_mono // self.states, len(graph["blocks"])
        if not self.triphones:
            return np.tile(np.arange(P * S, dtype=np.int32), (K, 1))
        if self.tree is None:
            raise ValueError("an Aligner with triphones has no tree before `fit`")
        ctx = triphone_contexts(graph, self.phone_ids, S)[::S]            # (l, p, r, 0) of every block
        bnd, ci = len(self.phone_ids), [self.phone_ids[p] for p in (SIL, SP, SPN)]
        free = np.isin(ctx[:, 1], ci)[:, None] | np.isin(np.arange(P), ci)[None, :]
        keys = np.empty((K, P, S, 4), np.int64)                            # (p, s, l, r), the order `tree_leaves` takes
        keys[..., 0] = np.arange(P)[None, :, None]
        keys[..., 1] = np.arange(S)[None, None, :]
        keys[..., 2] = np.where(free, bnd, ctx[:, 0][:, None])[:, :, None]
        keys[..., 3] = np.where(free, bnd, ctx[:, 2][:, None])[:, :, None]
        t = self.tree
        return tree_leaves(t["question"], t["yes"], t["no"], t["leaf"], t["member"], keys, S).reshape(K, P * S).astype(np.int32)

    def score(self, feats, lens, graphs, speakers=None, segmental=False):
        """`align` with the confidence scores of the "Confidence" paragraph -> ([frames per block] as `align` returns them,
        [`utterance_scores` dict per utterance]).  The per-frame arrays (own, best, arg, state, class: 28 bytes a frame) come back
        from the device, the block and utterance means are taken on the host in ascending t.  `segmental`: every dict also gets
        the numbers of the "Segmental scores" paragraph: `seg` (n_blocks, 3) = (gop_seg, rival, margin) per block, NaN for a block
        of 0 frames, `V` (n_blocks, P) and the utterance's `gop_seg`; without it nothing more is launched or returned."""
        x, lens, G, bp, end, vit = self._decode(feats, lens, graphs, speakers)
        frames = backtrack(bp, lens, G, end).cpu().numpy()
        state, cls = path(bp, lens, G, end)
        if self.mixtures == 1:
            tables = (torch.ones(self.n_classes, 1, dtype=torch.float64, device=self.device), self.mu.unsqueeze(1), self.var.unsqueeze(1))
        else:
            tables = (self.gw, self.gmu, self.gvar)
        own, best, arg = frame_scores(x, lens, cls, *tables)
        state, cls, own, best, arg, vit = (v.cpu().numpy() for v in (state, cls, own, best, arg, vit))
        phone = self.class_phone()
        out = [utterance_scores(G.graphs[b], state[b, :n], cls[b, :n], own[b, :n], best[b, :n], arg[b, :n], phone, vit[b])
               for b, n in enumerate(lens)]
        if segmental:
            S, P = self.states, self.n_mono // self.states
            seg = np.zeros((len(graphs), max(G.nbmax, 1), 2), np.int32)
            cand = np.full((len(graphs), max(G.nbmax, 1), P * S), -1, np.int32)
            for b, (g, n) in enumerate(zip(graphs, lens)):
                seg[b, :len(g["blocks"])] = segment_table(g, state[b, :n])
                cand[b, :len(g["blocks"])] = self.candidates(g)
            arc = np.stack([np.log(self.loop), np.log(1.0 - self.loop)], 1) if self.transitions else np.zeros((self.n_classes, 2))
            dev = self.device
            V = segment_scores(x, lens, _up(seg, dev), _up(cand, dev).reshape(len(graphs), -1, P, S), *tables, _up(arc, dev)).cpu().numpy()
            for b, g in enumerate(graphs):
                nb = len(g["blocks"])
                out[b]["V"] = V[b, :nb].copy()
                out[b]["seg"], out[b]["gop_seg"] = segment_reductions(g, seg[b, :nb], out[b]["V"])
        return [frames[b, :len(g["blocks"])].copy() for b, g in enumerate(graphs)], out

    def options(self):
        """The constructor's keyword arguments (without the device, the questions file and the phone table)."""
        return {"n_classes": self.n_mono, "dim": self.dim, "states": self.states, "mixtures": self.mixtures, "mix_iters": self.mix_iters,
                "min_split_occ": self.min_split_occ, "lda": self.lda, "splice": self.splice, "lda_iters": self.lda_iters,
                "fmllr": self.fmllr, "fmllr_rounds": self.fmllr_rounds, "fmllr_iters": self.fmllr_iters, "fmllr_sweeps": self.fmllr_sweeps,
                "fmllr_min_frames": self.fmllr_min_frames, "triphones": self.triphones, "tri_iters": self.tri_iters,
                "tri_min_occ": self.tri_min_occ, "tri_min_gain": self.tri_min_gain, "transitions": self.transitions}

    def save(self, path, phone_names, feature_config, speaker_names=None, bigram=None):
        """The trained model as one .npz (no pickled objects): every table `align` and `score` use (mu, var, or with mixtures gw, gmu,
        gvar, ncomp; the LDA's P, o; the speaker transforms W; the tree's arrays; loop, opt; floor), the constructor options, the phone
        table in id order, the feature configuration the model was trained under (`recognize.feature_config`), with fmllr the
        speaker names in index order, the bigram counts of `recognize.phone_bigram` (or none) and MODEL_VERSION."""
        phone_names = [str(p) for p in phone_names]
        if len(phone_names) * self.states != self.n_mono:
            raise ValueError(f"{len(phone_names)} phone names for a model of {self.n_mono // self.states} phones")
        if self.lda and self.P is None or self.fmllr and self.W is None or self.triphones and self.tree is None:
            raise ValueError("the model has not been trained: `fit` comes before `save`")
        host = lambda t: t.cpu().numpy()                                                   # noqa: E731
        out = {"version": np.array(MODEL_VERSION), "options": np.array(json.dumps(self.options())),
               "features": np.array(json.dumps(dict(feature_config))), "phones": np.array(phone_names),
               "floor": np.asarray(self.floor, np.float64), "loop": np.asarray(self.loop, np.float64), "opt": np.asarray(self.opt, np.float64)}
        if self.mixtures == 1:
            out.update(mu=host(self.mu), var=host(self.var))
        else:
            out.update(gw=host(self.gw), gmu=host(self.gmu), gvar=host(self.gvar), ncomp=np.asarray(self.ncomp, np.int64))
        if self.lda:
            out.update(P=host(self.P), o=host(self.o))
        if self.fmllr:
            names = [str(s) for s in (speaker_names if speaker_names is not None else [])]
            if len(names) != self.n_spk:
                raise ValueError(f"a model with fmllr has {self.n_spk} speaker transforms, {len(names)} speaker names were given")
            out.update(W=host(self.W), speakers=np.array(names))
        if self.triphones:
            t = self.tree
            out.update({"tree_" + k: np.asarray(t[k]) for k in ("question", "yes", "no", "leaf", "member")})
            out.update(tree_names=np.array([str(n) for n in t["names"]]), tree_numbers=np.array([t["gain"], t["n_items"], t["n_leaves"]], np.float64))
        if bigram is not None:
            out["bigram"] = np.asarray(bigram, np.float64)
        with open(path, "wb") as f:                                        # np.savez would append .npz to a bare name
            np.savez(f, **out)

    @classmethod
    def load(cls, path, device="cuda"):
        """The `Aligner` a file of `save` holds: its `align` and `score` return the bits of the original's.  The file's metadata are
        attributes: phone_names, feature_config, speaker_names (None without fmllr), bigram (None when the file has none)."""
        with np.load(path, allow_pickle=False) as f:
            d = {k: f[k] for k in f.files}
        if "version" not in d or int(d["version"]) != MODEL_VERSION:
            raise ValueError(f"{path} is not a model file of format {MODEL_VERSION}")
        opts, names = json.loads(str(d["options"])), [str(p) for p in d["phones"]]
        al = cls(device=device, phone_ids={p: i for i, p in enumerate(names)} if opts["triphones"] else None, **opts)
        al.phone_names, al.feature_config = names, json.loads(str(d["features"]))
        al.speaker_names = [str(s) for s in d["speakers"]] if al.fmllr else None
        al.bigram = d.get("bigram")
        al.floor, al.loop, al.opt = d["floor"], d["loop"], d["opt"]
        al.n_classes = len(al.loop)
        if al.mixtures == 1:
            al._set(d["mu"], d["var"])
        else:
            al.gw, al.gmu, al.gvar, al.ncomp = _up(d["gw"], al.device), _up(d["gmu"], al.device), _up(d["gvar"], al.device), d["ncomp"]
        if al.lda:
            al.P, al.o = _up(d["P"], al.device), _up(d["o"], al.device)
        if al.fmllr:
            al.W, al.n_spk = _up(d["W"], al.device), d["W"].shape[0]
        if al.triphones:
            gain, n_items, n_leaves = d["tree_numbers"]
            al.tree = {**{k: d["tree_" + k] for k in ("question", "yes", "no", "leaf", "member")}, "names": [str(n) for n in d["tree_names"]],
                       "gain": float(gain), "n_items": int(n_items), "n_leaves": int(n_leaves)}
        return al


MODEL_VERSION = 1
TRAINING_DEFAULTS = dict(states=2, iters=12, mixtures=1, mix_iters=4, lda=0, splice=3, lda_iters=4, fmllr=0, fmllr_rounds=2, fmllr_iters=2,
                         fmllr_sweeps=20, fmllr_min_frames=500, triphones=0, tri_iters=4, tri_min_occ=100, tri_min_gain=0.0, questions=None,
                         transitions=0)


def _load_for(model, dev, config, phone_ids, speakers, given):
    """The model file `build(model=...)` decodes with, after its refusals: training options beside it, a phone table, feature
    settings or a speaker it was not trained with -> (Aligner, speaker name -> its index in the model)."""
    from .recognize import feature_config
    extra = sorted(k for k, v in given.items() if v != TRAINING_DEFAULTS[k])
    if extra:
        raise ValueError(f"training options ({', '.join(extra)}) cannot be given together with a model file: it is not trained again")
    al = Aligner.load(model, dev)
    table = sorted(phone_ids, key=phone_ids.get)
    if table != al.phone_names:
        here, there = set(table) - set(al.phone_names), set(al.phone_names) - set(table)
        raise ValueError(f"the lexicon's phone table is not the model's: only in the lexicon {sorted(here)}, only in the model {sorted(there)}"
                         if here or there else "the lexicon's phone table is the model's in another order")
    fc = feature_config(config)
    if fc != al.feature_config:
        diff = ", ".join(f"{k} {fc[k]} (model: {al.feature_config.get(k)})" for k in fc if fc[k] != al.feature_config.get(k))
        raise ValueError(f"the config's feature settings are not the model's: {diff}")
    ids = {name: i for i, name in enumerate(speakers)}
    if al.fmllr:
        unknown = [s for s in speakers if s not in al.speaker_names]
        if unknown:
            raise ValueError(f"the model has no fmllr transform for the speakers {unknown} (it was trained with {al.speaker_names})")
        ids = {name: al.speaker_names.index(name) for name in speakers}
    return al, ids


# ------------------------------------------------------------------------------------------------ the corpus pass
def batches_by_bytes(frames, states, dim, budget, mixtures=1, splice_dim=0, fmllr_dim=0, transitions=0, seg_phones=0, block_states=2):
    """`ragged.greedy_batches` of (frames, states) under `budget` bytes of device buffers: E, alpha / gamma and backpointers (17 B per
    cell), features, partials; with `mixtures` = M > 1 also the responsibilities (8 M B per cell) and M times the partials; with
    `splice_dim` = D_s > 0 (LDA) also the spliced frames, D_s doubles per frame, and their partials while the statistics are taken
    (the scatter workspace, at most 82 MB for any batch, is not counted); with `fmllr_dim` = D > 0 also the frame weights c, h and
    the adapted frames, 3 D doubles per frame (the accumulation workspace, at most 141 MB and 16 B per utterance, is not counted);
    with `transitions` also the arc costs w and the second partial table xi, 3 + 5 doubles per state; with `seg_phones` = P > 0
    (segmental scores, `block_states` = S states per block) also, per block, the segment (8 B), its P S candidate classes (4 B
    each) and its P values of V (8 B each)."""
    if mixtures == 1:
        base = lambda n, T, J: n * (T * J * 17 + T * dim * 8 + J * (1 + 2 * dim) * 8)       # noqa: E731
    else:
        base = lambda n, T, J: n * (T * J * (17 + 8 * mixtures) + T * dim * 8 + J * mixtures * (1 + 2 * dim) * 8)  # noqa: E731
    cost = base if not splice_dim else lambda n, T, J: base(n, T, J) + n * (T * splice_dim * 8 + J * (1 + 2 * splice_dim) * 8)
    if fmllr_dim:
        lda_cost = cost
        cost = lambda n, T, J: lda_cost(n, T, J) + n * T * 3 * fmllr_dim * 8               # noqa: E731
    if transitions:
        plain_cost = cost
        cost = lambda n, T, J: plain_cost(n, T, J) + n * J * (3 + 5) * 8                  # noqa: E731
    if seg_phones:
        arcs_cost = cost
        cost = lambda n, T, J: arcs_cost(n, T, J) + n * (J // block_states) * (8 + seg_phones * (4 * block_states + 8))  # noqa: E731
    return ragged.greedy_batches(list(zip(frames, states)), budget, cost)


def build(config, device="cuda", states=2, iters=12, overwrite=False, batch_bytes=8 << 30, resident_bytes=16 << 30,
          batch_seconds=1800.0, num_workers=8, mixtures=1, mix_iters=4, lda=0, splice=3, lda_iters=4, fmllr=0, fmllr_rounds=2,
          fmllr_iters=2, fmllr_sweeps=20, fmllr_min_frames=500, triphones=0, tri_iters=4, tri_min_occ=100, tri_min_gain=0.0,
          questions=None, transitions=0, scores=None, g2p=None, seg_scores=0, save_model=None, model=None):
    """Align every `{raw_path}/{speaker}/{basename}.wav` that has a `.lab` and write its TextGrid.  Returns (written, skipped,
    log-likelihood per frame of every pass); `skipped` lists (speaker, basename, reason).  `scores` = a path: decoding goes through
    `Aligner.score` and one JSON object per written utterance goes to that file (the "Confidence" paragraph): speaker, basename,
    frames, scored_frames, viterbi, loglik, gop, match and phones = [label, start_s, end_s, loglik, gop, match] per written interval.
    `g2p` = a `fastspeech2_amd.g2p.G2P` model or the path of one: out-of-lexicon words get its pronunciation instead of `spn`
    (`pronounce_oov`, one batched decode of the corpus's OOV words before any graph is built); the count is printed.
    `seg_scores` = 1 (needs `scores`): the "Segmental scores" paragraph; every phone entry becomes [label, start_s, end_s, loglik, gop,
    match, gop_seg, rival_label, margin] and the utterance object gains gop_seg.  With 0 the scores file is what it was.
    `save_model` = a path: after `fit` the model goes to that file (`Aligner.save`) with the phone table, the feature settings, the
    speaker names and the bigram counts of the decoded alignments (fastspeech2_amd/recognize.py).  `model` = such a file: nothing
    is trained (the history is []), the corpus is aligned with the loaded model; training options beside it, a lexicon whose
    phone table is not the model's, other feature settings or, with fmllr, a speaker the model has no transform for are
    ValueErrors before any audio is read."""
    from . import audio as Audio
    from .preprocess import load_wav
    dev = ragged.require_device(torch.device(device), "fastspeech2_amd.align")
    if seg_scores not in (0, 1) or (seg_scores and scores is None):
        raise ValueError(f"seg_scores must be 0 or 1 and needs `scores`, got {seg_scores} with scores = {scores}")
    raw, out_dir = config["path"]["raw_path"], os.path.join(config["path"]["preprocessed_path"], "TextGrid")
    pp = config["preprocessing"]
    sr, hop, n_mel = pp["audio"]["sampling_rate"], pp["stft"]["hop_length"], pp["mel"]["n_mel_channels"]
    _, Ds, Dt = check_options(2 * n_mel, mixtures, mix_iters, lda, splice, lda_iters, fmllr, fmllr_rounds, fmllr_iters, fmllr_sweeps,
                              fmllr_min_frames, triphones, tri_iters, tri_min_occ, tri_min_gain, transitions)  # before any file is read
    Df = Dt if fmllr else 0
    speakers = sorted(d for d in os.listdir(raw) if os.path.isdir(os.path.join(raw, d)))
    if fmllr and len(speakers) * Df * (Df + 1) * (Df + 2) * 8 > resident_bytes:
        raise ValueError(f"the fmllr statistics of {len(speakers)} speakers in {Df} dimensions take "
                         f"{len(speakers) * Df * (Df + 1) * (Df + 2) * 8} bytes, more than resident_bytes = {resident_bytes}")
    speaker_ids = {name: i for i, name in enumerate(speakers)}
    lexicon = read_lexicon(config["path"]["lexicon_path"])
    phone_ids = phone_table(lexicon)
    aligner = None
    if model is not None:
        if save_model is not None:
            raise ValueError("save_model and model are not given together: a loaded model is not trained")
        given = dict(states=states, iters=iters, mixtures=mixtures, mix_iters=mix_iters, lda=lda, splice=splice, lda_iters=lda_iters,
                     fmllr=fmllr, fmllr_rounds=fmllr_rounds, fmllr_iters=fmllr_iters, fmllr_sweeps=fmllr_sweeps,
                     fmllr_min_frames=fmllr_min_frames, triphones=triphones, tri_iters=tri_iters, tri_min_occ=tri_min_occ,
                     tri_min_gain=tri_min_gain, questions=questions, transitions=transitions)
        aligner, speaker_ids = _load_for(model, dev, config, phone_ids, speakers, given)
        states, mixtures, transitions, fmllr = aligner.states, aligner.mixtures, aligner.transitions, aligner.fmllr
        Ds, Df = aligner.splice_dim, (aligner.lda or 2 * n_mel) if fmllr else 0
    if seg_scores and len(phone_ids) > max_seg_phones():
        raise ValueError(f"seg_scores takes at most {max_seg_phones()} phones, the lexicon has {len(phone_ids)}")
    if triphones:
        check_leaves(triphones, len(phone_ids) * states)
        real = len(phone_ids) - 3                                          # the item table: at most R S (R + 1)^2 + 3 S rows of 1 + 2 D
        table = (real * states * (real + 1) ** 2 + 3 * states) * (1 + 2 * Dt) * 8
        if table > resident_bytes:
            raise ValueError(f"the item table of {real} phones with {states} states in {Dt} dimensions may take {table} bytes, more "
                             f"than resident_bytes = {resident_bytes}")
        if questions is not None:
            read_questions(questions, phone_ids)                           # refuses a bad file before any work
    stft = Audio.TacotronSTFT(pp["stft"]["filter_length"], hop, pp["stft"]["win_length"], n_mel, sr, pp["mel"]["mel_fmin"],
                              pp["mel"]["mel_fmax"])

    entries = []
    for speaker in speakers:
        for name in sorted(os.listdir(os.path.join(raw, speaker))):
            if name.endswith(".wav") and os.path.exists(os.path.join(raw, speaker, name[:-4] + ".lab")):
                entries.append((speaker, name[:-4]))
    tg = lambda e: os.path.join(out_dir, e[0], e[1] + ".TextGrid")                       # noqa: E731
    existing = [e for e in entries if os.path.exists(tg(e))]
    if existing and not overwrite:
        raise FileExistsError(f"{len(existing)} TextGrids exist already (first: {tg(existing[0])}); pass --overwrite to replace them")

    if g2p is not None:
        if isinstance(g2p, str):
            from .g2p import G2P
            g2p = G2P.load(g2p, dev)
        transcripts = []
        for e in entries:
            with open(os.path.join(raw, e[0], e[1] + ".lab"), encoding="utf-8") as f:
                transcripts.append(words_of(f.readline()))
        lexicon, taken, left = pronounce_oov(transcripts, lexicon, phone_ids, g2p)
        print(f"{taken} out-of-lexicon words pronounced by the g2p model, {left} left as {SPN}")

    def read(e):
        wav = np.clip(load_wav(os.path.join(raw, e[0], e[1] + ".wav"), sr), -1.0, 1.0).astype(np.float32)
        with open(os.path.join(raw, e[0], e[1] + ".lab"), encoding="utf-8") as f:
            return wav, words_of(f.readline())

    # stage 1: wav + lab on a host thread pool, log-mel + features on the GPU per ragged batch of audio, features back to the host
    items, skipped = [], []
    batch_samples = int(batch_seconds * sr)

    staging = ragged.Staging()

    def extract(chunk):
        for batch in ragged.greedy_batches([(len(c[1]),) for c in chunk], batch_samples, ragged.padded_samples):
            wavs = [chunk[k][1] for k in batch]
            staging.pack(wavs)
            mel, _, fr = stft.mel_spectrogram_ragged(staging.to(dev), [len(w) for w in wavs])
            x = features(mel.contiguous(), fr.tolist()).cpu()
            for r, k in enumerate(batch):
                e, _, words, graph = chunk[k]
                items.append({"entry": e, "words": words, "graph": graph, "x": x[r, :int(fr[r])].clone()})

    with ThreadPoolExecutor(max_workers=max(1, num_workers)) as pool:
        step = max(64, 8 * num_workers)
        for c0 in range(0, len(entries), step):
            chunk = []
            for e, (wav, words) in zip(entries[c0:c0 + step], pool.map(read, entries[c0:c0 + step])):
                if not words:
                    skipped.append((e[0], e[1], "empty transcript"))
                    continue
                graph = utterance_graph(words, lexicon, phone_ids, states)
                T = len(wav) // hop + 1
                if len(wav) <= pp["stft"]["filter_length"] // 2 or T < graph["mandatory"]:
                    skipped.append((e[0], e[1], f"{T} frames for {graph['mandatory']} mandatory states"))
                elif len(graph["sid"]) > max_states():
                    skipped.append((e[0], e[1], f"{len(graph['sid'])} states exceed the supported {max_states()}"))
                else:
                    chunk.append((e, wav, words, graph))
            if chunk:
                extract(chunk)
    for s in skipped:
        print("skipped {}/{}: {}".format(*s))
    if not items:
        return 0, skipped, []

    # stage 2: ragged batches under the byte budget; the packed features stay on the device when the corpus fits
    D = 2 * n_mel
    frames, nstates = [it["x"].shape[0] for it in items], [len(it["graph"]["sid"]) for it in items]
    resident = sum(frames) * D * 8 <= resident_bytes
    packed = []
    for batch in batches_by_bytes(frames, nstates, D, batch_bytes, mixtures, Ds, Df, transitions, len(phone_ids) if seg_scores else 0, states):
        feats = torch.zeros(len(batch), max(frames[i] for i in batch), D, dtype=torch.float64)
        for r, i in enumerate(batch):
            feats[r, :frames[i]] = items[i]["x"]
            items[i]["x"] = None
        packed.append((feats.to(dev) if resident else feats, [frames[i] for i in batch], [items[i]["graph"] for i in batch], batch))
    spk_of = lambda batch: [speaker_ids[items[i]["entry"][0]] for i in batch] if fmllr else None    # noqa: E731
    history = []
    if aligner is None:
        aligner = Aligner(len(phone_ids) * states, D, states, dev, mixtures, mix_iters, lda=lda, splice=splice, lda_iters=lda_iters,
                          fmllr=fmllr, fmllr_rounds=fmllr_rounds, fmllr_iters=fmllr_iters, fmllr_sweeps=fmllr_sweeps,
                          fmllr_min_frames=fmllr_min_frames, triphones=triphones, tri_iters=tri_iters, tri_min_occ=tri_min_occ,
                          tri_min_gain=tri_min_gain, questions=questions, phone_ids=phone_ids if triphones else None,
                          transitions=transitions)
        history = aligner.fit([p[:3] for p in packed], iters, [spk_of(p[3]) for p in packed] if fmllr else None)

    written = 0
    phone_names = sorted(phone_ids, key=phone_ids.get)
    heard = []                                                             # per utterance, the phones of the blocks with frames
    none_if_nan = lambda v: None if v != v else float(v)                                 # noqa: E731
    sink = open(scores, "w", encoding="utf-8") if scores is not None else None
    try:
        for feats, lens, graphs, batch in packed:
            if sink is None:
                got, conf = aligner.align(feats, lens, graphs, spk_of(batch)), [None] * len(batch)
            else:
                got, conf = aligner.score(feats, lens, graphs, spk_of(batch), segmental=bool(seg_scores))
            for i, fr, sc in zip(batch, got, conf):
                e = items[i]["entry"]
                os.makedirs(os.path.join(out_dir, e[0]), exist_ok=True)
                wd, ph, xmax = intervals(items[i]["graph"], items[i]["words"], fr, hop, sr)
                write_textgrid(tg(e), wd, ph, xmax)
                written += 1
                if save_model is not None:
                    heard.append(block_phones(items[i]["graph"])[np.nonzero(fr)[0]])
                if sink is not None:
                    rows = sc["blocks"][np.nonzero(fr)[0]]                 # the written intervals: the blocks with frames
                    line = {"speaker": e[0], "basename": e[1], **{k: sc[k] for k in ("frames", "scored_frames", "viterbi", "loglik", "gop", "match")},
                            "phones": [[p, s0, s1] + [float(v) for v in r] for (s0, s1, p), r in zip(ph, rows)]}
                    if seg_scores:
                        line["gop_seg"] = none_if_nan(sc["gop_seg"])
                        for entry, (g_, q, m) in zip(line["phones"], sc["seg"][np.nonzero(fr)[0]]):
                            entry += [none_if_nan(g_), None if q != q else phone_names[int(q)], none_if_nan(m)]
                    sink.write(json.dumps(line, allow_nan=False) + "\n")
    finally:
        if sink is not None:
            sink.close()
    if save_model is not None:
        from .recognize import feature_config, phone_bigram
        aligner.save(save_model, phone_names, feature_config(config), speakers[:aligner.n_spk] if fmllr else None,
                     phone_bigram(heard, len(phone_names))[0])
    return written, skipped, history
