/* azg.h -- C-ABI of the MI355X-native batched self-play engine (libazg_hip.so).
 *
 * The reference (cestpasphoto/alpha-zero-general) is 100% Python and has NO FFI; its boundary for this path is duck
 * typing.  This header is the C boundary a binding for the reference would call: every entry point
 * names the reference interface it replaces (file:line under the reference root).  The Python host side in
 * alpha-zero-general_amd/ mirrors Game.py / MCTS.py / Coach.py on top of exactly these functions through ctypes.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; azg_last_error() gives the message (thread-local).
 *   - `*_dev` pointers are DEVICE pointers (e.g. torch.Tensor.data_ptr()); `stream` is a hipStream_t passed as void*
 *     (NULL = default stream).  Kernels are enqueued on that stream and the call returns without synchronising, so
 *     they can be captured in a HIP graph.  Functions without a stream argument synchronise the device.
 *   - states are int8, C-contiguous, byte-identical to the reference's board.tobytes()
 *     (splendor/SplendorLogicNumba.py:207-219, santorini/SantoriniLogicNumba.py:658-665).
 *   - no callbacks into the host language; one host thread per forest handle.
 *
 * RNG contract (shared with oracle/rng.c):
 *     mix64(x): x^=x>>30; x*=0xBF58476D1CE4E5B9; x^=x>>27; x*=0x94D049BB133111EB; x^=x>>31
 *     raw(seed, stream, counter) = mix64(mix64(mix64(seed ^ 0x9E3779B97F4A7C15) + stream) + counter)
 *     u01 = (raw >> 11) * 2^-53;   stream = global game index, counter = per-game draw count.
 *   Per ply a self-play game draws: u_full (MCTS.py:58), u_pick (Coach.py:289-292), then whatever
 *   make_move(random_seed=0) consumes (SplendorLogicNumba.py:311-315).  u_pick drives np.random.choice(len(p), p=p) as NumPy does it
 *   (searchsorted of the normalised cumulative sum).  With temperature == 0 (Coach.py:278-283) the reference calls np.random.choice
 *   twice -- the unweighted choice among the maxima, k = floor(u_pick * n_maxima), then the weighted choice on the one-hot result --
 *   so a SECOND uniform is consumed after u_pick (fixture tests/golden/episode_splendor2_temp0.npz, played by the reference).
 */
#ifndef AZG_H
#define AZG_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { AZG_SPLENDOR = 0, AZG_SANTORINI = 1, AZG_AZUL = 2, AZG_MINIVILLES = 3, AZG_ABALONE = 4, AZG_TLP = 5, AZG_BOTANIK = 6, AZG_AKROPOLIS = 7, AZG_SMALLWORLD = 8 };
#define AZG_MAX_PLAYERS 5
#define AZG_MAX_UNIVERSES 8

const char* azg_last_error(void);
const char* azg_version(void);
int azg_device_count(void);
int azg_set_device(int device);

/* GameSwitcher.import_game + Game.getBoardSize/getActionSize/getNumberOfPlayers (GameSwitcher.py:15-24, Game.py:27-42).
   variant: Splendor = NUMBER_PLAYERS (2..4, splendor/SplendorGame.py:9); Santorini = NB_GODS (1 or 11,
   santorini/SantoriniConstants.py:19); Azul = 2 players (azul/AzulGame.py:9); Minivilles = NUMBER_PLAYERS (2..4,
   minivilles/MinivillesGame.py:9); Abalone = the two module constants of abalone/AbaloneLogicNumba.py:5-6 in one word: bits 0-1 the starting layout (0 or
   1 Belgian Daisy, 2 German Daisy, 3 classic), bit 2 (value 4) ENABLE_DYNAMIC_KOMI -- init draws one uniform u and stores floor(2 u) in
   misc[0][3], the bit decides a score tie at the round limit and flips with the seats; any other bit is refused; The Little Prince =
   NUMBER_PLAYERS (3..5, thelittleprince/TLPGame.py:9); Botanik = 2 players; Akropolis = N_PLAYERS (2..4,
   akropolis/AkropolisConstants.py:3); Smallworld = NUMBER_PLAYERS (2..4, smallworld/SmallworldConstants.py).  0 = the shipped constant. */
int azg_game_info(int game, int variant, int* state_bytes, int* action_size, int* num_players, int* rows, int* cols);

/* ---- batched env step (one wavefront per state) ------------------------------------------------------------------
   Replace the per-call <G>Game adaptor methods (splendor/SplendorGame.py:28-48, santorini/SantoriniGame.py:28-48). */
/* Game.getValidMoves(board, player) -> bool[A]            out_valid_dev: u8[n][A] */
int azg_env_valid_moves(int game, int variant, const int8_t* states_dev, const int32_t* players_dev, int n,
                        uint8_t* out_valid_dev, void* stream);
/* Game.getNextState(board, player, action, random_seed) -> (board', next_player).  random_seed==0 draws from the RNG
   contract with (rng_seed, stream = stream0 + i, counter = counters_dev[i]) and advances counters_dev[i]. */
int azg_env_next_state(int game, int variant, const int8_t* states_dev, const int32_t* players_dev,
                       const int32_t* actions_dev, const int64_t* random_seeds_dev, int n, int8_t* out_states_dev,
                       int32_t* out_next_players_dev, uint64_t rng_seed, uint64_t stream0, uint64_t* counters_dev,
                       void* stream);
/* Game.getGameEnded(board, next_player) -> f32[P] ; getScore -> i32[P] ; getRound -> i32 */
int azg_env_game_ended(int game, int variant, const int8_t* states_dev, const int32_t* next_players_dev, int n,
                       float* out_ended_dev, int32_t* out_scores_dev, int32_t* out_round_dev, void* stream);
/* Game.getCanonicalForm(board, player) */
int azg_env_canonical(int game, int variant, const int8_t* states_dev, const int32_t* players_dev, int n,
                      int8_t* out_states_dev, void* stream);
/* Game.getInitBoard() for n games (Board.init_game); RNG contract with stream = stream0 + i, counter from 0;
   out_counters_dev (optional) receives the number of draws consumed. */
int azg_env_init_boards(int game, int variant, int n, int8_t* out_states_dev, uint64_t rng_seed, uint64_t stream0,
                        uint64_t* out_counters_dev, void* stream);
/* Game.getSymmetries (Game.py:96-109; Board.get_symmetries SplendorLogicNumba.py:255-301, SantoriniLogicNumba.py:578-653,
   AzulLogicNumba.py:310-331) for n (state, pi, valids) triples: form k of triple t goes to row [t][k] of
   out_states int8[n][max_sym][S], out_pi f32[n][max_sym][A], out_valids u8[n][max_sym][A]; out_count i32[n] = forms
   written (the reference's order: identity first; <= 10 + 2P for Splendor, 8 for Santorini, 120 for Azul).
   Coach.executeEpisode records every form of every full-search ply (Coach.py:66-69). */
int azg_env_symmetries(int game, int variant, const int8_t* states_dev, const float* pi_dev, const uint8_t* valids_dev, int n,
                       int max_sym, int8_t* out_states_dev, float* out_pi_dev, uint8_t* out_valids_dev,
                       int32_t* out_count_dev, void* stream);
/* The same with a random source, for games whose get_symmetries is itself random (The Little Prince, TLPLogicNumba.py:177-272:
   np.random.shuffle of players / market cards / planet slots, duplicate states dropped; <= 2P + 1 forms): triple t draws from
   the RNG contract's stream (rng_seed, stream0 + t), counter from 0, with shuffle(x) = Fisher-Yates from the top
   (j = floor(u (i + 1)) for i = len-1 .. 1).  Other games ignore the two arguments; azg_env_symmetries = (0, 0). */
int azg_env_symmetries_ex(int game, int variant, const int8_t* states_dev, const float* pi_dev, const uint8_t* valids_dev, int n,
                          int max_sym, int8_t* out_states_dev, float* out_pi_dev, uint8_t* out_valids_dev,
                          int32_t* out_count_dev, uint64_t rng_seed, uint64_t stream0, void* stream);

/* ---- one move per game without a search (one wavefront per game) ----------------------------------------------------
   Replaces <G>Players.RandomPlayer.play (mode 0), np.argmax of a policy or of getActionProb's vector (mode 1: Arena.py:79, pit.py's
   raw-policy players) and np.random.choice(A, p=pi) (mode 2) for T games at once.  probs_dev f32[T][A] (modes 1, 2), valid_dev u8[T][A]
   as azg_env_valid_moves writes it (NULL = every action valid), active_dev u8[T] (NULL = every game): a game with active == 0 keeps its
   actions_out_dev[t] and its counters_dev[t].
     mode 0: u = RNG contract (rng_seed, stream0 + t, counters_dev[t]); the floor(u nv)-th of the nv valid actions in index order.
     mode 1: the first index of the maximum of probs over the valid actions; a NaN never wins; no candidate -> 0.
     mode 2: the same u; weights = probs where valid and > 0, else 0; the first index whose cumulative weight (f64, index order) exceeds
             u * total; when rounding leaves none (or the total is 0), the last valid index.
   Modes 0 and 2 advance counters_dev[t] by exactly one, also when the game has no valid action (the action is then 0);
   counters_dev == NULL draws at counter 0.  T == 0 launches nothing; a bad mode, or NULL probs in modes 1 and 2, is an error. */
int azg_pick_actions(int mode, const float* probs_dev, const uint8_t* valid_dev, int T, int A, const uint8_t* active_dev,
                     uint64_t rng_seed, uint64_t stream0, uint64_t* counters_dev, int32_t* actions_out_dev, void* stream);

/* ---- random playouts to the end of the game, one launch (one wavefront per playout) -----------------------------------
   Replaces <G>Players.RandomPlayer.play looped by Arena.playGame (Arena.py:67-84) and launcher.py's random play: k playouts from each
   of n states, every move uniform among the valid ones, the state on chip from the first ply to the last.  Row r = t * k + j is
   playout j of state t and owns the RNG contract's stream (rng_seed, stream0 + r), from counters_dev[r] (NULL: from 0, nothing written
   back).  A ply, in this order:
     1. getGameEnded(board, player): any entry non-zero -> the playout is over, status 0;
     2. plies == max_plies -> status 1 (cap), the result row is all zeros;
     3. getValidMoves(board, player): none -> status 2, the result row is all zeros;
     4. one uniform u; the min(floor(u nv), nv - 1)-th of the nv valid actions in index order (azg_pick_actions, mode 0);
     5. getNextState(board, player, action, random_seed = 0) on the same stream: a game's dice, refills and card draws follow the pick's
        draw; plies += 1.
   This is what the ply-by-ply loop azg_env_game_ended / azg_env_valid_moves / azg_pick_actions(mode 0) / azg_env_next_state computes when
   its pick and its env step share (stream0, counters_dev).  At the end counters_dev[r] holds the stream's next counter.
   SEAT FRAME: out_ended_dev is in the seat numbering of the INPUT board -- the env step never renumbers seats.  For a canonical leaf
   (the player to move is seat 0) entry 0 is therefore the result of the player to move, which is what NeuralNet.predict's v[0] means
   (MCTS.py:131,153,175-178).
   active_dev u8[n] (NULL = every state): the k rows of a state with active == 0 keep their outputs and their counters.  Optional
   outputs may be NULL; entries of out_actions_dev past a row's plies are left as they were.  n == 0 launches nothing.  An unknown
   game / variant, k < 1, max_plies outside 1 .. 65535 or a NULL required output is an error and launches nothing.  No synchronisation
   and no allocation: the call can sit inside a captured round. */
int azg_env_playouts(int game, int variant,
                     const int8_t* states_dev,      /* [n][S] */
                     const int32_t* players_dev,    /* [n], NULL = player 0 everywhere */
                     const uint8_t* active_dev,     /* [n], NULL = every row */
                     int n, int k, int max_plies,
                     uint64_t rng_seed, uint64_t stream0,
                     uint64_t* counters_dev,        /* [n*k] or NULL (start at 0, not written back) */
                     float*   out_ended_dev,        /* [n][k][P]  getGameEnded(final board, final player) */
                     int32_t* out_plies_dev,        /* [n][k] */
                     uint8_t* out_status_dev,       /* [n][k]  0 finished, 1 cap, 2 no valid move */
                     int8_t*  out_states_dev,       /* [n][k][S] or NULL: the final boards */
                     int32_t* out_players_dev,      /* [n][k] or NULL: the player to move at the end */
                     int32_t* out_actions_dev,      /* [n][k][max_plies] or NULL: the moves; entries past plies untouched */
                     void* stream);

/* ---- one-ply lookahead: all successors of n positions, one launch (waves_per_state wavefronts per position) -----------
   The loop of <G>Players.GreedyPlayer.play (splendor/SplendorPlayers.py:76-79, abalone/AbalonePlayers.py:195-201) -- for every valid
   move, getNextState and getScore -- for n positions at once.  For state t:
     out_valid_dev[t] = getValidMoves(board, player), as azg_env_valid_moves writes it;
   and for every valid action a, row [t][a] of the other outputs is exactly what these two calls give:
     azg_env_next_state on that row with action a and random_seed = 0, on the RNG contract's stream (rng_seed, stream0 + t) from
       counters_dev[t] (NULL: from 0)                              -> out_states_dev[t][a] (optional), out_next_player_dev[t][a];
     azg_env_game_ended(next state, next player)                   -> out_ended_dev[t][a], out_scores_dev[t][a] (getScore of all P seats).
   Every candidate of a state starts from the SAME counter: the call is a peek.  counters_dev is never written and nothing is advanced.
   SEAT FRAME: the input board's -- the env step never renumbers seats (Game.getNextState returns (player + 1) % P without a swap), as
   in azg_env_playouts.  For a canonical board (the mover is seat 0) entry 0 of a row is the mover's.
   Rows of invalid actions keep what the buffers held; so do ALL rows of a state with active == 0, out_valid_dev[t] included.
   The work of a state is dealt out over waves_per_state wavefronts (the valid action of rank r goes to wave r mod waves_per_state); the
   result does not depend on it.  n == 0 launches nothing.  An unknown game / variant, waves_per_state outside 1 .. 64 or a NULL required
   output is an error and launches nothing.  No synchronisation and no allocation. */
int azg_env_lookahead(int game, int variant,
                      const int8_t* states_dev,       /* [n][S] */
                      const int32_t* players_dev,     /* [n], NULL = player 0 everywhere */
                      const uint8_t* active_dev,      /* [n], NULL = every state */
                      int n, int waves_per_state,     /* 1 .. 64 */
                      uint64_t rng_seed, uint64_t stream0,
                      const uint64_t* counters_dev,   /* [n] or NULL (every peek from 0); never written */
                      uint8_t* out_valid_dev,         /* [n][A] */
                      int32_t* out_scores_dev,        /* [n][A][P] */
                      float*   out_ended_dev,         /* [n][A][P] */
                      int32_t* out_next_player_dev,   /* [n][A] */
                      int8_t*  out_states_dev,        /* [n][A][S] or NULL: the successor boards */
                      void* stream);

/* ---- the greedy players' candidate sets (one wavefront per position) ---------------------------------------------------
   canonical_states_dev int8[n][S] are CANONICAL boards (the mover is seat 0), valid_dev u8[n][A] and scores_dev i32[n][A][P] what
   azg_env_lookahead wrote for them.  out_candidates_dev[t][a] = 1 where a is a move the player may take, else 0; a position without a
   valid move gives an all-zero row; a position with active == 0 keeps its row.  The move itself is
   azg_pick_actions(mode 0, probs NULL, valid = candidates): uniform among the candidates, one draw.
   rule AZG_GREEDY_REFERENCE -- <G>Players.GreedyPlayer of the reference, quirks included; Splendor, Azul and Abalone only (any other
   game: error "the reference defines no greedy player for this game"):
     Splendor (splendor/SplendorPlayers.py:68-90): s_a = score of seat 1 after move a -- the reference reads seat 1 of a board that
       getNextState did not renumber, i.e. the OPPONENT's score; M = max s_a over the valid moves; init = getScore(board, 0).  M != init:
       the valid a with s_a == M.  Otherwise the valid ids in [0, 12); if none, those in [30, 60); if none, every valid id.
     Abalone (abalone/AbalonePlayers.py:182-206): the valid a of maximal score[1] - score[0] after the move (same seat reading).
     Azul (azul/AzulPlayers.py:36-70): no lookahead (scores_dev may be NULL), one candidate from the board alone: the first valid move of
       maximal (to_line, -to_floor) with to_line = min(line + 1 - board[11][line], n), to_floor = n - to_line, n = board[3 + a / 30][colour]
       (line 5: to_line = 0) -- except that the reference's `if not best_move` also replaces a kept move 0, so move 0 is the candidate
       only when no other move is valid.
   rule AZG_GREEDY_LEAD -- this project's own, any game: the valid a of maximal score[0] - max over p >= 1 of score[p] after the move
     (the mover's lead; what the reference's players intend). */
#define AZG_GREEDY_REFERENCE 0
#define AZG_GREEDY_LEAD 1
int azg_greedy_candidates(int game, int variant, int rule, const int8_t* canonical_states_dev, const uint8_t* valid_dev,
                          const int32_t* scores_dev, int n, const uint8_t* active_dev, uint8_t* out_candidates_dev, void* stream);

/* ---- validation losses on a net's outputs (one wavefront per example row) -------------------------------------------
   Replaces the loss half of GenericNNetWrapper.evaluate (:159-177; loss_pi / loss_v :179-190) for B examples: pi_dev f32[B][A] are
   PROBABILITIES as the engine nets return them, v_dev f32[B][P], target_pi_dev f32[B][A], z_dev / q_dev f32[B][P], active_dev u8[B]
   (NULL = every row).  Per row, in f64:
     rows_dev[b][0]  = sum over the actions with t > 0 of t (log t - log max(pi, FLT_MIN))   (F.kl_div's xlogy convention: an action
                       with t == 0 adds exactly 0, whatever pi is);
     rows_dev[b][1]  = sum_p ((z + q_weight q) / (1 + q_weight) - v)^2                        (q_weight as the f32 it is passed as);
     flags_dev[b][0] = 1 when the first-index argmax of target_pi is the first-index argmax of pi (np.argmax; a NaN never wins);
     flags_dev[b][1] = the number of actions with t > 0 and pi < FLT_MIN -- where the floor was applied: an engine probability can
                       underflow to 0, and the caller sees that here instead of an inf.
   A row with active == 0 writes zeros and counts for nothing.  Every lane of the row's wave sums its actions l, l + 64, ... in index
   order and the lanes are combined in one fixed tree: a row's numbers are bit-identical from call to call and do not depend on B.
   totals_dev f64[4] = the sums of the four columns over the rows, by a second launch of one wave inside this call (rows l, l + 64, ...
   in order, then the same tree; no atomics); with accumulate != 0 they are ADDED to what totals_dev holds, so a validation set
   evaluated in chunks needs one host read at the end.  loss_pi = totals[0] / n, loss_v = totals[1] / (n P).
   rows_dev, flags_dev and totals_dev are REQUIRED: the caller owns them (azg_amd.nnet.eval_losses allocates them), the call owns no
   memory.  B == 0 launches the totals pass alone (without accumulate it zeroes totals_dev) and needs no other pointer.  B < 0, A < 1,
   P outside 1 .. 8, B or A above 2^31 - 65, q_weight <= -1 (or NaN) or a NULL required pointer is an error and launches nothing.  No
   synchronisation and no allocation: the call can sit inside a captured graph. */
int azg_eval_losses(const float* pi_dev, const float* v_dev, const float* target_pi_dev, const float* z_dev, const float* q_dev,
                    const uint8_t* active_dev, int B, int A, int P, float q_weight, double* rows_dev, int32_t* flags_dev,
                    double* totals_dev, int accumulate, void* stream);

/* ---- the training step's batches (GenericNNetWrapper.train :44-92) without the host: draw, gather, score ------------------------
   Three calls that replace np.random.choice (:57), the five fancy-index reads (:58-63) and loss_pi / loss_v (:179-190) with their
   backward pass down to the net's outputs.  Each enqueues on `stream` and returns; nothing is allocated, nothing is read back. */
/* np.random.choice(n, batch, replace=False) for n_steps steps in ONE launch (one wave per step): ids_out_dev int32[n_steps][batch].
   Row s is a function of (rng_seed, stream0 + s, n, batch) alone, on the RNG contract above, with exactly `batch` uniforms and no
   rejection -- a Fisher-Yates shuffle over a virtual identity:
       p = identity on [0, n);   for i = 0 .. batch - 1:   m = n - i,   j = i + min(floor(u01(rng_seed, stream0 + s, counter i) * m), m - 1),
                                                           ids[i] = p[j],   p[j] = p[i]
   (the product in f64).  Every ordered tuple of distinct indices is equally likely.  1 <= batch <= 8192, batch <= n < 2^31 and
   n_steps >= 0 are required, anything else is an error and launches nothing; n_steps == 0 launches nothing and needs no pointer. */
int azg_train_sample_ids(int64_t n, int batch, int n_steps, uint64_t rng_seed, uint64_t stream0, int32_t* ids_out_dev, void* stream);
/* Rows ids_dev[0 .. B) of the five example columns in one launch (one wave per row): boards_dev int8[n][S], pi_dev f32[n][A], z_dev /
   q_dev f32[n][P], valids_dev u8[n][A] -> out_boards_dev int8[B][S], out_pi_dev f32[B][A], out_z_dev / out_q_dev f32[B][P], out_valids_dev
   u8[B][A] holding valids != 0 as 0 / 1 bytes (a bool tensor's storage).  Rows may start at any byte offset (S = 75, A = 21).  An id
   outside [0, n) cannot be refused without reading the ids back: the row's content is then undefined (no memory outside the columns is
   touched).  n < 1, B < 0, S < 1, A < 1, P outside 1 .. 8 or a NULL pointer (with B > 0) is an error and launches nothing. */
int azg_train_gather(const int8_t* boards_dev, const float* pi_dev, const float* z_dev, const uint8_t* valids_dev, const float* q_dev,
                     const int32_t* ids_dev, int n, int B, int S, int A, int P, int8_t* out_boards_dev, float* out_pi_dev, float* out_z_dev,
                     uint8_t* out_valids_dev, float* out_q_dev, void* stream);
/* loss_pi + loss_v (:179-190) of a training batch on the module's outputs -- log_pi_dev f32[B][A] are LOG-probabilities (masked actions
   carry -1e8), v_dev f32[B][P] -- and the gradient of L = loss_pi + v_coeff * loss_v with respect to both.  Two launches: one wave per
   row, then one wave for the totals.
     rows_dev[b][0] = sum over the actions with t > 0 of t (log t - log_pi)   (t == 0 adds exactly 0 and gets the gradient 0, whatever
                      log_pi holds);            rows_dev[b][1] = sum_p (t_v - v)^2,   t_v = (z + q_weight q) / (1 + q_weight)
     out_dev[0] = sum_b rows[b][0] / B ('batchmean'),   out_dev[1] = sum_b rows[b][1] / (B P)
   in f64 from the f32 inputs; lanes take entries in index order and are combined in one fixed tree, so the numbers are the same bits
   in every call.  The gradients are f32, operation for operation what autograd computes on the GPU for the expression of train.train
   (a tensor divided by a host scalar is multiplied by the scalar's f32 reciprocal there):
     grad_log_pi_dev[b][a] = -(t (1 / B)),      grad_v_dev[b][p] = -((v_coeff (1 / (B P))) (2 (t_v - v))),   t_v = (z + q_weight q) (1 / (1 + q_weight))
   with 1 + q_weight in f32.  When B and B P are powers of two every scale is exact.  B < 1, A < 1, P outside 1 .. 8, B or A above
   2^31 - 65, q_weight <= -1 (or NaN) or a NULL pointer is an error and launches nothing. */
int azg_train_losses(const float* log_pi_dev, const float* v_dev, const float* target_pi_dev, const float* z_dev, const float* q_dev,
                     int B, int A, int P, float q_weight, float v_coeff, float* grad_log_pi_dev, float* grad_v_dev, double* rows_dev,
                     double* out_dev, void* stream);
/* torch.optim.AdamW under OneCycleLR (:49-51, :81-82) for every parameter in ONE launch, the step number taken
   from device memory: nothing in the call changes from step to step, so a captured graph can replay it.
     segs_dev[n_segs]: one entry per parameter tensor -- p (updated), g (its gradient), m / v (the two moments, updated), numel < 2^31;
     chunks_dev[n_chunks]: { seg, first }: one workgroup of 256 lanes updates elements [first, min(first + 2048, numel)) of segment seg;
                       first is a multiple of 2048.  A chunk that names no segment or starts outside it touches nothing;
     table_dev f32[total_steps][8]: row s = { 1 - lr_s wd, 1 - beta1_s, beta2, 1 - beta2, lr_s / (1 - beta1_s^(s+1)), sqrt(1 - beta2^(s+1)),
                       eps, 0 }, the scalars of optimiser step s computed on the host in f64 and cast once (train.onecycle_adamw_table);
     step_dev: the counter; every workgroup reads it once and uses row clamp(*step_dev, 0, total_steps - 1).
   Per element in f32, each operation rounded on its own (no contraction), in the order of torch's foreach AdamW, r = the row:
     p = p r0;   m = m + r1 (g - m);   v = v r2;   v = v + (g g) r3;   d = sqrt(v) / r5 + r6;   p = p - r4 (m / d)
   16-byte loads and stores where a chunk is whole and its segment's four pointers are 16-byte aligned, single floats otherwise.
   A NULL pointer, n_segs < 1, n_chunks < 1 or total_steps < 1 is an error and launches nothing. */
typedef struct azg_adamw_seg { float* p; const float* g; float* m; float* v; int64_t numel; } azg_adamw_seg;
typedef struct azg_adamw_chunk { int32_t seg, first; } azg_adamw_chunk;
int azg_train_adamw(const azg_adamw_seg* segs_dev, int n_segs, const azg_adamw_chunk* chunks_dev, int n_chunks, const float* table_dev,
                    int total_steps, const int64_t* step_dev, void* stream);
/* *step_dev += 1 in a one-wave launch of its own: enqueued behind azg_train_adamw, no workgroup of the update can see the new value. */
int azg_train_step_advance(int64_t* step_dev, void* stream);

/* ---- an iteration's records -> dense example rows, one launch (one wavefront per record) --------------------------------------------
   Replaces Coach.executeEpisode's loop over getSymmetries (Coach.py:66-69) for n drained records: group g expands source record
   order_dev[g] (NULL: record g) into its symmetric forms -- the forms, their order (identity first) and their number are those of
   azg_env_symmetries_ex with max_sym = the game's maximum -- and form k becomes ROW first_row_dev[g] + k of the five output columns:
   out_states int8[rows][S], out_pi f32[rows][A], out_valids u8[rows][A], and the record's z / q replicated into out_z / out_q
   f32[rows][P].  Only rows inside [row_begin, row_end) are written; a form whose row lies outside (first_row_dev may be negative) is
   skipped, but it is still counted and still consumes its draws.  out_count_dev int32[n] = the forms of group g, window or not.
   first_row_dev == NULL is the COUNT pass: nothing but out_count_dev is written (the output columns may be NULL) and the counts are
   those of the write pass, draws included; the caller's prefix sum over them gives first_row_dev.
   Games with random forms draw group g from the RNG contract's stream (rng_seed, stream0 + g), counter from 0 -- the GROUP index, not
   the source record's: a caller that reorders with order_dev gets the streams of the same call on pre-permuted inputs.
   An order_dev entry outside [0, n) gives the group no form (count 0) and reads nothing.  n == 0 launches nothing.  NULL inputs with
   n > 0, a NULL output column in a write pass with a non-empty window, an unknown game / variant or row_end < row_begin is an error
   and launches nothing.  No synchronisation and no allocation. */
int azg_examples_expand(int game, int variant,
                        const int8_t* states_dev, const float* pi_dev, const float* z_dev, const uint8_t* valids_dev, const float* q_dev, int n,
                        const int32_t* order_dev,       /* NULL or int32[n]: group g expands source record order[g] */
                        const int64_t* first_row_dev,   /* NULL = count only; else int64[n]: destination row of form 0 of group g (may be negative) */
                        int64_t row_begin, int64_t row_end,   /* only rows in [row_begin, row_end) are ever written */
                        int8_t* out_states_dev, float* out_pi_dev, float* out_z_dev, uint8_t* out_valids_dev, float* out_q_dev,
                        int32_t* out_count_dev,         /* int32[n]: forms of group g, in both modes */
                        uint64_t rng_seed, uint64_t stream0, void* stream);
/* The other half of the call above: a training batch computed from the RECORDS, so that the expanded rows need not be stored (one
   wavefront per batch row, one launch).  The n records are the five columns [n][S | A | P | A | P]; three index columns place their
   forms on an axis of VIRTUAL rows: form k of record g is virtual row first_row_dev[g] + k, the record's live rows end at row_end_dev[g]
   (exclusive; NON-DECREASING in g -- a record with no live row repeats its predecessor's value), and its forms draw from the RNG
   contract's stream (rng_seed, streams_dev[g]), counter from 0 (streams_dev == NULL: stream g).
   For batch row b: r = ids_dev[b]; g = the lowest record with row_end_dev[g] > r (binary search); k = r - first_row_dev[g]; row b of the
   five outputs (laid out as azg_train_gather's) then holds exactly the bytes azg_examples_expand writes to row first_row[g] + k when a
   group expands that record on that stream: the same candidates in the same order (identity first), for the built games the same draws
   and the same duplicate dropping -- at most the game's maximum number of forms is rebuilt per batch row.  z and q are the record's own;
   valids are written as 0 / 1 bytes (valids != 0, as azg_train_gather writes them).
   An id that no record owns (r < 0, r >= row_end_dev[n - 1]) or a k outside the record's forms cannot be refused without reading the
   ids back: the row's content is then undefined (no memory outside the columns is touched).  An unknown game / variant, B < 0, n < 1
   with B > 0 or a NULL pointer other than streams_dev (with B > 0) is an error and launches nothing; B == 0 launches nothing.  No
   synchronisation and no allocation: the call can be captured in a graph. */
int azg_train_gather_forms(int game, int variant,
                           const int8_t* states_dev, const float* pi_dev, const float* z_dev, const uint8_t* valids_dev, const float* q_dev,
                           const int64_t* first_row_dev,   /* int64[n]: virtual row of form 0 of record g (may lie below its first live row) */
                           const int64_t* row_end_dev,     /* int64[n]: one past the last live virtual row of record g; non-decreasing */
                           const uint64_t* streams_dev,    /* uint64[n] or NULL (= g) */
                           int n, const int32_t* ids_dev, int B,
                           int8_t* out_boards_dev, float* out_pi_dev, float* out_z_dev, uint8_t* out_valids_dev, float* out_q_dev,
                           uint64_t rng_seed, void* stream);

/* ---- forest: T independent MCTS trees, one wavefront per tree ----------------------------------------------------
   Replaces MCTS (MCTS.py:19-261) for a batch of trees and, in self-play mode, Coach.executeEpisode (Coach.py:37-84). */
typedef struct azg_forest_cfg {
    int game, variant;
    int n_trees;                 /* concurrent games on this GPU */
    int node_capacity;           /* nodes per tree (arena); GC keeps it bounded in self-play */
    int row_capacity_bytes;      /* per-tree row heap; 0 = auto */
    /* args.* of the reference (main.py:120-156, pit.py:49-57) */
    int numMCTSSims;
    double cpuct, fpu;
    int universes;
    double prob_fullMCTS;
    int ratio_fullMCTS;
    int forced_playouts;
    double dirichletAlpha;       /* 0 = no root noise; noise samples are supplied by the caller (torch Dirichlet) */
    double temperature[3];       /* [begin, end, root-softmax] (Coach.py:266-271, MCTS.py:148) */
    double tempThreshold;
    uint64_t rng_seed;
    uint64_t stream0;            /* global index of tree 0 (rank * n_trees in multi-GPU runs) */
    int max_examples;            /* capacity of the on-device example ring (self-play mode) */
    int level_budget;            /* max descent levels per tree per azg_forest_select launch; a deeper simulation is parked
                                    and resumed by the next launch (0 = unlimited).  Pure scheduling: results identical. */
    int work_budget;             /* cap on the work of one tree in one azg_forest_select launch, in level units (one descent
                                    level = 1, one frontier-edge resolution = 5; 0 = unlimited): a launch lasts as long as
                                    its slowest tree, so the few trees with a very deep or transposition-heavy simulation
                                    are parked at a level boundary and resume in the next launch.  Pure scheduling. */
    int gc_high_water_pct;       /* self-play clean-up (the reference's MCTS.py:86-91, every > 20 rounds): a tree whose arena holds more
                                    than this share of node_capacity when its next search begins is cleaned up first -- not only when
                                    the arena could not take another search -- so the arena keeps headroom and can be sized for the
                                    LIVE tree instead of live + many plies of dead nodes.  0 = only at exhaustion (rounds 1-3).  Which
                                    nodes survive does not depend on when the clean-up runs: results identical. */
} azg_forest_cfg;

typedef struct azg_forest azg_forest;

int azg_forest_create(const azg_forest_cfg* cfg, azg_forest** out);           /* MCTS.__init__ MCTS.py:24-47 */
int azg_forest_destroy(azg_forest* f);
size_t azg_forest_device_bytes(const azg_forest* f);

/* MCTS.reset_all_search_trees (MCTS.py:199-203) */
int azg_forest_reset(azg_forest* f, void* stream);

/* --- host-driven mode: the pieces of MCTS.getActionProb (MCTS.py:49-103) --- */
/* begin a search on every tree: canonical roots int8[T][S]; full_dev u8[T] (1 = full search, 0 = fast search, 2 = this
   tree sits the search out and keeps its contents -- e.g. the opponent's turn in an Arena) or NULL (all full).
   The tree is reused if the root state is already a node (MCTS.py:125-126). */
int azg_forest_begin_search(azg_forest* f, const int8_t* roots_dev, const uint8_t* full_dev, void* stream);
/* one lock-step round, part 1: every tree runs simulations until it needs the net (one leaf per tree) or has finished
   its numMCTSSims.  Writes the leaf batch for NeuralNet.predict (NeuralNet.py:32-43):
   leaf_states int8[T][S], leaf_valid u8[T][A], needs_eval u8[T].   MCTS.search :105-175 */
int azg_forest_select(azg_forest* f, int8_t* leaf_states_dev, uint8_t* leaf_valid_dev, uint8_t* needs_eval_dev,
                      const double* root_noise_dev /* f64[T][|noise_stride|] or NULL */, int noise_stride, void* stream);
/* root noise (MCTS.py:64,187-197): applied on simulation 0 of full searches when root_noise_dev != NULL.
   noise_stride > 0: rows hold iid Gamma(dirichletAlpha,1) variates, normalised on device over the root's n_valid
   first entries (== rng.dirichlet([alpha]*n_valid)); noise_stride < 0: rows already hold a Dirichlet sample over the
   valid actions (parity tests inject the reference's own sample), stride = -noise_stride.
   root_noise_dev == NULL with noise_stride == -1: the engine draws the Gamma variates itself (counter-based stream keyed
   by rng_seed / game stream / simulation count; cfg.dirichletAlpha > 0, or < 0 for the automatic 10/n_valid).
   root_noise_dev == NULL with noise_stride == -2 (self-play): same device sampler, but run by the next
   azg_selfplay_advance launch instead of a launch of its own; a tree whose root noise is pending sits out the selects
   in between (same per-tree event sequence, so results do not depend on how often advance is launched). */
/* part 2 + part 1 in one launch (self-play): first the expansion + backup of the leaves the PREVIOUS select handed out
   (pi / v as for azg_forest_expand_backup; leaf_valid must still hold that select's masks), then the next descent.  Saves
   a launch and its cold header reads per round; results are identical to expand_backup followed by select.
   noise_stride: 0 = no root noise, -2 = device sampler run by azg_selfplay_advance (see azg_forest_select). */
int azg_forest_select_fused(azg_forest* f, int8_t* leaf_states_dev, uint8_t* leaf_valid_dev, uint8_t* needs_eval_dev,
                            const float* pi_dev, const float* v_dev, int noise_stride, void* stream);
/* The per-CU form of the self-play round for Splendor 2 players + the V80 net (csrc/azg_fused.hip.h): ONE launch runs `rounds` rounds of
       azg_forest_select_fused  ->  azg_nn_v80_forward_h2 on the leaf batch
   with one 16-wave workgroup per 16 trees doing both -- every wave descends one tree, then the same waves evaluate the workgroup's 16
   leaves -- so that a round of a CU waits for the slowest of ITS 16 trees instead of the slowest of all T, and nothing is launched
   between the rounds (what the reference does with a lock ring of N game threads around one inference batch, Coach.py:117-144).
   Arguments as for those two calls (same buffers, same 43-pointer weight table + 16 descale factors); per-tree results are identical
   bit for bit to `rounds` times the two calls (tests/test_gpu_selfplay.py).  azg_selfplay_advance is launched by the caller between
   launches, as between rounds of the two-kernel form. */
int azg_forest_rounds_v80_h2(azg_forest* f, int8_t* leaf_states_dev, uint8_t* leaf_valid_dev, uint8_t* needs_eval_dev, float* pi_dev,
                             float* v_dev, int noise_stride, const void* const* w, const float* descale_host, int rounds, void* stream);
/* measurement: phase times of that kernel since the last reset, from the 100 MHz wall clock read inside the kernel, averaged over the
   workgroups -- out[0] = select phase of a round (a workgroup waits for the slowest of its 16 trees), out[1] = net phase, out[2] = a
   wave's own descent, all in microseconds per round; out[3] = rounds measured.  (bench.py's roofline uses out[0]: there is no launch
   of the descent alone to put HIP events around.) */
int azg_forest_rounds_profile(azg_forest* f, double* out4, int reset);

/* The ASYNCHRONOUS TREE PIPELINE form of the self-play round for Splendor 2 players + the V80 net (csrc/azg_async.hip.h): games search
   while other games sit in the net -- what the reference's lock ring of N game threads around one inference server does
   (Coach.py:117-144, GenericNNetWrapper.py:122-157).  ONE call launches two persistent kernels that run concurrently: `n_sel` descent
   workgroups (16 waves; each owns a fixed share of the trees, a free wave takes whichever of them has its pi / v, runs the expansion +
   backup + next descent of azg_forest_select_fused and queues the leaf) and `n_net` net workgroups (each takes up to 16 queued leaves --
   fewer after `batch_wait_ticks` x 10 ns of waiting --, runs the forward of azg_nn_v80_forward_h2 on them and hands the trees back).
   A "call" of a tree is what one round of the two-kernel form does for it (expansion + backup of its evaluated leaf, then descents until a
   leaf needs the net, the search ends or the work budget parks it).  shared_budget == 0: every tree has exactly `rounds` calls, then the
   kernels end -- results are a function of `rounds` alone.  shared_budget != 0: the kernels end when the trees TOGETHER have had rounds x T
   calls; a fast tree gets more of them, no tree waits for the slowest at the end of the launch (per-game results are the same, how far
   each game gets is not fixed).  What azg_selfplay_advance does between rounds -- the move, the example record, the restart, the
   clean-up, the next search, the root noise -- happens inside, per tree, the moment its search is finished: no call of
   azg_selfplay_advance is needed (or harmful) between launches.  n_net + n_sel must not exceed the CUs of the device (every workgroup has to
   be resident; <= 0: a default split); the split may change from call to call.  Per-tree results are identical bit for bit to
   `rounds` x (azg_forest_select_fused -> azg_selfplay_advance -> azg_nn_v80_forward_h2) with shared_budget == 0 (tests/test_gpu_selfplay.py).
   leaf_valid_dev u8[T][A], needs_eval_dev u8[T], pi_dev f32[T][A], v_dev f32[T][P]: as for azg_forest_select_fused (the leaf states
   travel through a buffer the forest owns).
   Determinism: with shared_budget != 0 the GAMES played are the same as with per-tree budgets (a tree's sequence of calls is its own),
   but how many of them are finished after N launches depends on GPU timing; callers that need "the examples after N runs" to be a function
   of the seed use shared_budget == 0 (Python: SelfPlayEngine(deterministic=True) or AZG_DETERMINISTIC=1; 3-4 % slower).
   Exclusive use: every workgroup of both kernels must be resident, so the device's CUs must not be held by other kernels for long (two
   engines on one GPU split the CUs with n_net / n_sel).
   Time-outs and recovery (csrc/azg_async.hip.h "Recovery"): a wave that finds nothing to do for AZG_ASYNC_TIMEOUT_MS (default 50) ends
   the launch.  That is a launch that ENDS EARLY, not an error: on this platform a few workgroups are occasionally not scheduled for
   about a second; the leaves they held are re-queued by the next launch (a small kernel in front of it), nothing is evaluated twice or
   lost, and the early end is counted (azg_forest_async_profile out[17] / [18]: ended by a descent / a net wave, [26] ticket ranges
   abandoned, [27] leaves re-queued).  With per-tree budgets every tree keeps the calls it has not run yet and a call of this function
   launches the pipeline TWICE -- the second launch grants nothing and only runs what the first left over -- so the "exactly `rounds` calls
   per tree" contract holds at every return whether or not the first launch ended early (both ending early: the next call catches up).
   Eight early ends in a row set error bit 128 (azg_selfplay_stats.errors): a pipeline that cannot make progress fails loudly.
   rounds: 1 .. 2^24 - 1 with a shared budget, 1 .. 2^22 - 1 with per-tree budgets; rounds == 0 with per-tree budgets: a catch-up launch only
   (Python's SelfPlayEngine(deterministic=True).run() issues these until the early-end counters [17] / [18] stop moving); < 0, or 0 with
   a shared budget: the call does nothing.  Early ends are counted by the net kernel's workgroup 0, which leaves only when the launch is over. */
int azg_forest_async_rounds_v80_h2(azg_forest* f, uint8_t* leaf_valid_dev, uint8_t* needs_eval_dev, float* pi_dev, float* v_dev,
                                   int noise_stride, const void* const* w, const float* descale_host, int rounds, int n_net, int n_sel,
                                   int batch_wait_ticks, int shared_budget, void* stream);
/* The same pipeline for a Santorini no-gods forest with the V89 net: w = the 14 device pointers and descale of azg_nn_conv5_forward_h2, 8
   leaves per forward; default split 49 / 64 of the CUs for the net.  Everything else as above. */
int azg_forest_async_rounds_conv5_h2(azg_forest* f, uint8_t* leaf_valid_dev, uint8_t* needs_eval_dev, float* pi_dev, float* v_dev,
                                     int noise_stride, const float* const* w, float descale, int rounds, int n_net, int n_sel,
                                     int batch_wait_ticks, int shared_budget, void* stream);
/* ... and for Splendor 3 / 4 players, Azul, Minivilles 2 - 4 players and The Little Prince 3 - 5 players with their MobileNet-1d nets: geometry
   (AZG_NET_SPLENDOR3 / 4, AZG_NET_AZUL, AZG_NET_MINIVILLES2 / 3 / 4, AZG_NET_TLP3 / 4 / 5), w (43 device pointers) and descale (16 host floats) as
   for azg_nn_mb1d_forward_h2; 8 (Splendor, TLP 3 players) / 16 (Azul, Minivilles) / 6 (TLP 4 / 5 players) leaves per forward.  A geometry that
   is not the forest's game and player count is an error that names both; nothing is launched.  Minivilles and TLP are STOCHASTIC (dice,
   market refills): the descent draws them from the tree's own counter stream in the order of the two-kernel rounds, so per-tree results
   are identical bit for bit to those rounds here as well (shared_budget == 0).  Opt-in from Python (SelfPlayEngine(async_pipe=True)). */
int azg_forest_async_rounds_mb1d_h2(azg_forest* f, int geometry, uint8_t* leaf_valid_dev, uint8_t* needs_eval_dev, float* pi_dev, float* v_dev,
                                    int noise_stride, const void* const* w, const float* descale_host, int rounds, int n_net, int n_sel,
                                    int batch_wait_ticks, int shared_budget, void* stream);
/* ... and for Smallworld 2 / 3 / 4 players (the player count is the forest's) with the V62 transformer: the lock ring of game threads
   around one inference server (Coach.py:117-144, GenericNNetWrapper.py:122-157) with SmallworldNNet.py nn_version 62 as the net.
   w = the 25 device pointers of azg_nn_sw62_forward (no descale), 4 / 3 / 2 leaves per forward (the samples of one k_sw62_net workgroup);
   default split 7 / 8 of the CUs for the net, fewer when the trees need more descent workgroups (at most 128 trees each).  Per-tree results
   are identical bit for bit to `rounds` x (azg_forest_select_fused -> azg_selfplay_advance -> azg_nn_sw62_forward) with shared_budget == 0.
   A null argument or a forest of another game: an error, nothing is launched.  Everything else as above. */
int azg_forest_async_rounds_sw62(azg_forest* f, uint8_t* leaf_valid_dev, uint8_t* needs_eval_dev, float* pi_dev, float* v_dev, int noise_stride,
                                 const float* const* w, int rounds, int n_net, int n_sel, int batch_wait_ticks, int shared_budget, void* stream);
/* measurement: counters of the pipeline since the last reset (ticks = 10 ns of the 100 MHz wall clock read inside the kernels):
   out[0] descents (select_tree calls), [1] ticks inside them, [2] ticks descent waves spent looking for a ready tree, [3] net batches,
   [4] leaves in them, [5] ticks inside the forward, [6] ticks net workgroups waited for leaves, [7] sum over leaves of (claimed by a net
   workgroup - queued), [8] sum over descents of (tree claimed - tree handed back by the net), [9] launches, [10] / [11] resident ticks
   summed over the select / net workgroups, [12] n_sel, [13] n_net, [17] / [18] launches ended early by a descent / net wave's time-out,
   [26] ticket ranges abandoned, [27] leaves re-queued at the start of a launch, [32..63] histogram of [7]'s waits in microseconds (last bucket: >= 31), [64..95] of [8]'s. */
#define AZG_ASYNC_NPROF 96
int azg_forest_async_profile(azg_forest* f, double* out96, int reset);

/* part 2: store (Ps, v) on the pending leaves and back the values up (MCTS.py:147-154,176-183).
   pi f32[T][A] are PROBABILITIES (exp of the net's log-softmax, GenericNNetWrapper.py:107,119), v f32[T][P].
   The leaf_valid buffer handed to the preceding azg_forest_select must still hold what that call wrote (the kernel maps
   entry j of a leaf to its j-th valid action through it). */
int azg_forest_expand_backup(azg_forest* f, const float* pi_dev, const float* v_dev, const double* root_noise_dev,
                             int noise_stride, void* stream);
/* number of trees that still have simulations to run (synchronises) */
int azg_forest_active(azg_forest* f, int* n_active);
/* MCTS.getActionProb epilogue (:67-103): probs f64[T][A] for temperature temp_dev f64[T] (or scalar temp if NULL),
   q f32[T][P], is_full u8[T].  Any output may be NULL. */
int azg_forest_action_probs(azg_forest* f, double temp, double* probs_dev, float* q_dev, uint8_t* is_full_dev,
                            void* stream);
/* root statistics for parity checks: Ns i32[T], Qs f32[T], Nsa i32[T][A], Qsa f64[T][A] (sentinel -42 where unvisited),
   Ps f32[T][A], n_nodes i32[T] */
int azg_forest_root_stats(azg_forest* f, int32_t* Ns_dev, float* Qs_dev, int32_t* Nsa_dev, double* Qsa_dev,
                          float* Ps_dev, int32_t* n_nodes_dev, void* stream);
/* whole-tree dump of one tree to HOST memory for parity tests (synchronises): for every node: state[S], flags,
   Ns, Qs, Es[P], and dense Nsa/Qsa/Ps[A].  Returns node count; arrays sized for max_nodes. */
int azg_forest_dump_tree(azg_forest* f, int tree, int max_nodes, int8_t* states, int32_t* Ns, float* Qs, float* Es,
                         int32_t* Nsa, double* Qsa, float* Ps, uint8_t* has_policy);

/* XCD-pinned streams (no reference counterpart: the reference time-slices N game threads on one core, Coach.py:117-144; here groups
   of games can run as independent select -> predict pipelines, selfplay.py): a HIP stream whose queue ASKS for the CUs of XCDs
   [xcd_first, xcd_first + xcd_count) of the current device only (hipExtStreamCreateWithCUMask; bit b of the mask = CU b / 8 of XCD
   b % 8).  Whether the mask is honoured is up to the platform: on the round-4 MI355X box (one partition over 8 XCDs) it was NOT -- the
   hardware deals a queue's workgroups round-robin over all XCDs; azg_testaids.h has a probe that shows where a launch really ran.  Pass the
   handle as `stream` to any call of this header. */
int azg_stream_create_xcd(int xcd_first, int xcd_count, void** out_stream);
int azg_stream_destroy(void* stream);
/* debug / tests: check the structural invariants of every tree on the host; returns the number of violations */
int azg_forest_validate(azg_forest* f, int verbose);

/* --- self-play mode: Coach.executeEpisode on device (Coach.py:37-84) --- */
/* start one game per tree (Board.init_game or the given init boards int8[T][S]) */
int azg_selfplay_start(azg_forest* f, const int8_t* init_boards_dev /* or NULL */, void* stream);
/* the same with (a) an RNG epoch: epoch 0 == azg_selfplay_start; another epoch re-keys every random stream of the forest, so
   the next wave of episodes of one Coach.learn run (Coach.py:150-215 draws fresh randomness every iteration) does not replay
   the previous one; (b) an episode quota = Coach.executeEpisodes' numEps (Coach.py:86-148): tree t plays quota / T (+1 for
   t < quota % T) games to their end and then idles -- every started game is finished and kept; 0 = restart forever; -1 = this
   forest plays no game (every tree idle: a group of a larger engine whose share of numEps is empty).
   Seed and quota are kernel arguments: HIP graphs that captured this forest's launches under another epoch / quota must be
   captured again. */
int azg_selfplay_start_ex(azg_forest* f, const int8_t* init_boards_dev /* or NULL */, uint64_t epoch, int64_t episode_quota,
                          void* stream);
/* sizeof(azg_forest_cfg) of this build: a binding compares it with its own declaration before it hands a cfg over */
int azg_forest_cfg_size(void);
/* to be called after expand_backup, every round or every few rounds: trees whose search finished sample the move
   (Coach.py:63,278-292), record the example (Coach.py:65-69), play it (Coach.py:71), detect the end (Coach.py:73-82),
   restart finished games, re-root and begin the next search -- all on device. */
int azg_selfplay_advance(azg_forest* f, void* stream);
/* trees that are still playing (synchronises): 0 once every tree has used up its episode quota (or stopped on an error) */
int azg_selfplay_active(azg_forest* f, int* n_active);
/* counters (synchronises): plies executed, games finished, simulations run, examples stored, error flags.
   errors = OR over trees: 1 node arena full, 2 record heap full, 4 descent deeper than 256, 8 bad state, 16 / 32 example ring / per-game
   record buffer full, 64 every pruned root count was 0 (numMCTSSims too small for the game's number of valid actions with
   forced_playouts: the reference divides 0 / 0 at MCTS.py:77-80,100-102 and raises).  A tree with an error is parked. */
typedef struct azg_selfplay_stats {
    uint64_t plies, games, sims, levels, expansions, sum_valid_visited, terminal_hits, examples, gc_runs, max_nodes,
        errors, sum_depth_at_expand,
        cyc_select, cyc_levels, cyc_edge, cyc_leaf,   /* (library built with -DAZG_CYC_COUNTERS only, else 0) shader-clock cycles summed over trees: whole k_select, descent levels,
                                                         frontier edge resolution (incl. leaf creation), leaf creation */
        cyc_seg[4],                                   /* frontier edge split: parent-state load, env step, canonical form +
                                                         hash, table probe */
        max_live_after_gc,                            /* most nodes of one tree that survived a clean-up: node_capacity must stay
                                                         above this + numMCTSSims */
        examples_dropped;                             /* records of finished games that did not fit the example ring (a game is
                                                         stored whole or not at all); != 0 also sets error bit 16 */
} azg_selfplay_stats;
int azg_selfplay_stats_get(azg_forest* f, azg_selfplay_stats* out);
/* drain finished-game examples: (board int8[S], pi f32[A], z f32[P], valids u8[A], q f32[P]) per record
   (Coach.py:76-82).  Returns count copied (<= max_records), device->device on `stream` then synchronises. */
int azg_selfplay_drain_examples(azg_forest* f, int max_records, int8_t* boards_dev, float* pi_dev, float* z_dev,
                                uint8_t* valids_dev, float* q_dev, int32_t* meta_dev /* i32[n][4] = (global game
                                stream, game index on it, ply, player) or NULL */, int* n_out, void* stream);

/* ---- policy/value nets: NeuralNet.predict for a whole leaf batch, every net in one launch (NeuralNet.py:32-43,
   GenericNNetWrapper.py:94-120; V80 network splendor/SplendorNNet.py:148-202,262-283,397-440) ---- */
/* The whole V80 forward (NeuralNet.predict for a leaf batch, SplendorNNet.py:397-440 / GenericNNetWrapper.py:94-110) in
   ONE launch, one workgroup pass per 16 samples: boards int8[B][56][7] -> first_layer + trunk block (output kept in LDS,
   two copies) -> policy head block + Flatten + Linear + ReLU + Linear + masked softmax -> pi f32[B][81]; value head block
   + Flatten + Linear + ReLU + Linear + tanh -> v f32[B][P].  f32 operands throughout: MFMA v_mfma_f32_16x16x4_f32 (exact f32
   == an fmaf chain).  w = 43 device pointers: {W0[64][64], b0[64]}, 3 x the 11 tensors of an InvertedResidual1d block
   (SplendorNNet.py:189-202: expand + depthwise + SE + project + residual; trunk, policy head, value head)
   {We[64][176], be[176], Wd[7][7], bn_scale[168], bn_bias[168], W1[176][48], b1[48], W2[48][176], b2[176], Wp[176][64],
   bp[64]}, {Wpi1[432][96], bpi1[96], Wpi2[96][96], bpi2[96]}, {Wv1[432][16], bv1[16], Wv2[P][P], bv2[P]}; zero padded,
   BatchNorm folded; the flatten index of Wpi1 / Wv1 rows is k = l*60 + c (c < 56).  Every matrix except Wd / Wv2 is stored in
   MFMA fragment order: frag[n/16][k/16][lane 0..63][j 0..3] = W[16*(k/16) + 4*(lane>>4) + j][16*(n/16) + (lane&15)] (one 1 KiB
   load per wave and K chunk); where K = 8 mod 16 (W0, We, W1, Wp) the last chunk holds its 8 rows as
   W[16*(k/16) + 2*(lane>>4) + j] in j = 0, 1.  Fixed to the V80 activations (trunk ReLU + mean squeeze, heads Hardswish + max
   squeeze). */
int azg_nn_v80_forward(const int8_t* boards_dev, const uint8_t* valid_dev, const float* const* w, int B, int P,
                       float* pi_dev, float* v_dev, void* stream);
/* The same forward with the expand GEMM of the three blocks on split-precision operands (every f32 value as three bf16 numbers
   hi + mid + lo, a product = the six bf16 MFMAs of relative weight >= 2^-24; f32-input MFMA runs at 1/16 of the bf16 rate on
   gfx950): the tile the blocks read lives in LDS as three bf16 planes, written split once by the producing epilogue; one copy of
   the trunk output serves both heads.  Only We (w[2], w[13], w[24]) differs: [11 column tiles][2 K chunks of 32][3 planes]
   [64 lanes][8] bf16 with element = W_plane[32*chunk + 8*(lane>>4) + j][16*tile + (lane&15)], K zero padded 56 -> 64. */
int azg_nn_v80_forward_split(const int8_t* boards_dev, const uint8_t* valid_dev, const float* const* w, int B, int P,
                             float* pi_dev, float* v_dev, void* stream);
/* The same forward (NeuralNet.predict for a leaf batch, SplendorNNet.py:397-440 / GenericNNetWrapper.py:94-110) on fp16 hi+lo
   split operands (every f32 weight / activation as hi = rn16(x), lo = rn16(x - hi): 22 significant bits; a product = three
   v_mfma_f32_16x16x32_f16) with TOKEN-MAJOR tiles, so that the depthwise token mix, its BN + activation, the squeeze and the SE
   scale run on MFMA accumulators in registers (csrc/nn_v80_h2.hip.h).  Same 1e-5 contract as azg_nn_v80_forward.
   w = the 43 slots of azg_nn_v80_forward with every matrix except Wd / Wv2 as h2 fragments: zero padded to K % 32 == 0,
   N % 16 == 0 -- W0[64][64], We[64][176], W1[192][48], W2[64][176], Wp[192][64], Wpi1[448][96] and Wv1[448][16] (row k =
   token*64 + c), Wpi2[96][96] -- scaled by a power of two 2^k per matrix and stored as
   [N/16 tiles][K/32 chunks][2 planes hi, lo][64 lanes][8] f16, element = W_plane[32*chunk + 8*(lane>>4) + j][16*tile + (lane&15)];
   vectors zero padded f32: b0[64], be / sd / bd / b2[176], b1[48], bp[64], bpi1 / bpi2[96], bv1[16].
   The token-mix matrices Wd[7][7] of the two Hardswish blocks (policy, value head) are passed DIVIDED BY 6: the kernel computes
   6 * Hardswish and leaves the 1/6 to the next linear step.
   descale (HOST array of 16 floats) = 2^-k / 64 for W0, {We, W1, W2, Wp} x (trunk, policy, value), Wpi1, Wpi2, Wv1. */
/* Activation range of the f16 x 2 ("h2") forwards -- azg_nn_v80_forward_h2, azg_nn_mb1d_forward_h2, azg_nn_conv5_forward_h2,
   azg_nn_s78_forward_h2: their LDS planes hold 64 * x as f16 (hi) + f16 (lo), so the 1e-5 contract holds for activations and
   residual-stream values |x| < 1023.  The reference's trained nets, float64 modules on the boards of reachable positions
   (tests/test_net_reachable_boards.py): The Little Prince 166 to 181 over its player counts (212 with 5 players on the early-game rows
   of netfwd_tlp5_v83.npz), Abalone 71 to 113 over its layouts, Santorini V78 89, every other shipped net at most 71; the stand-in
   weights of Minivilles 4p and Botanik reach 125 and 134.  Beyond the range the value SATURATES: the kernels run
   with the FP16_OVFL bit of the wave MODE register set, so an f16 conversion that overflows gives +-65504 instead of inf -- pi / v stay
   finite, never NaN (tests/test_nnet.py::test_h2_kernels_saturate_out_of_range_activations_gpu).  A net that may leave the range (e.g.
   a diverging training run) is evaluated with the f32-operand kernels (azg_nn_v80_forward / _mb1d_forward / _conv5_forward /
   _s78_forward; Python: h2=False), which have the full f32 range at 1/3 .. 1/2 of the speed. */
int azg_nn_v80_forward_h2(const int8_t* boards_dev, const uint8_t* valid_dev, const void* const* w, const float* descale_host,
                          int B, int P, float* pi_dev, float* v_dev, void* stream);
/* The whole MobileNetV3-1d forward (first layer, trunk block, policy block + head, value block + head) in one launch for
   the geometries of the reference's Splendor (SplendorNNet.py:259-283, n players: C = 32 + 10n + n^2 channels x 7 tokens)
   and Azul (AzulNNet.py:91-113: 23 channels x 6 tokens) nets, and of the shipped nets of Minivilles (MinivillesNNet.py:101-123,
   n players: C = 18 + 20n channels x 2 tokens) and The Little Prince (TLPNNet.py:175-196, n players: C = 1 + 18n channels x 15 tokens),
   every shipped player count -- the generic sibling of azg_nn_v80_forward.  An unknown geometry id returns an error and launches nothing.
   boards int8 [B][C][L], valid u8 [B][A] -> pi f32 [B][A] (probabilities), v f32 [B][P].  w = 43 device pointers:
   {W0, b0}, 3 x {We, be, Wd[L][L], bn_scale_d, bn_bias_d, W1, b1, W2, b2, Wp, bp} (trunk, policy head, value head),
   {Wpi1, bpi1, Wpi2, bpi2, Wv1, bv1, Wv2[P][P], bv2}; every matrix but Wd / Wv2 is zero-padded to multiples of 16 in both
   dimensions and stored in MFMA fragment order frag[N/16][K/16][64][4] = W[16c + 4*(lane>>4) + j][16nt + (lane&15)],
   every vector zero-padded to a multiple of 16; the rows of Wpi1 / Wv1 are indexed l*OS + c with OS = 16*ceil(max(C,
   policy-block channels)/16) + 4. */
enum { AZG_NET_SPLENDOR2 = 0, AZG_NET_SPLENDOR3 = 1, AZG_NET_SPLENDOR4 = 2, AZG_NET_AZUL = 3,
       AZG_NET_MINIVILLES2 = 4,   /* minivilles/MinivillesNNet.py:101-123 nn_version 82, 2 players: C = 58, L = 2, A = 21 */
       AZG_NET_TLP3 = 5,          /* thelittleprince/TLPNNet.py:175-196 nn_version 83, 3 players: C = 55, L = 15, A = 9 */
       AZG_NET_MINIVILLES3 = 6,   /* minivilles/MinivillesNNet.py:101-123 nn_version 82, 3 players: C = 78, L = 2, A = 21 */
       AZG_NET_MINIVILLES4 = 7,   /* minivilles/MinivillesNNet.py:101-123 nn_version 82, 4 players: C = 98, L = 2, A = 21 */
       AZG_NET_TLP4 = 8,          /* thelittleprince/TLPNNet.py:175-196 nn_version 83, 4 players: C = 73, L = 15, A = 16 */
       AZG_NET_TLP5 = 9 };        /* thelittleprince/TLPNNet.py:175-196 nn_version 83, 5 players: C = 91, L = 15, A = 25 */
int azg_nn_mb1d_forward(int geometry, const int8_t* boards_dev, const uint8_t* valid_dev, const float* const* w, int B,
                        float* pi_dev, float* v_dev, void* stream);
/* The same forward with every GEMM phase on f16 x 2 split-precision operands (hi + lo halves, three v_mfma_f32_16x16x32_f16 per
   K chunk of 32, fp32 accumulation: <= 1e-5 of the fp32 forward); the activations stay fp32 in the LDS and are split as they
   are read.  w: the same 43 pointers, every matrix but Wd / Wv2 as an azg_nn_v80_forward_h2 fragment array (K zero-padded to a
   multiple of 32: 16*ceil(K/16) rounded up; N to a multiple of 16); descale_host[16] as there. */
int azg_nn_mb1d_forward_h2(int geometry, const int8_t* boards_dev, const uint8_t* valid_dev, const void* const* w,
                           const float* descale_host, int B, float* pi_dev, float* v_dev, void* stream);
/* The Santorini ResNet (santorini/SantoriniNNet.py nn_version 88/89 :194-219,273-281: conv3x3(2->64)+BN+ReLU, n_blocks
   SimpleResBlocks :71-84, SimpleHead heads :17-40) in one launch.  boards int8 [B][5][5][3] (planes 0, 1 are the net's
   input), valid u8 [B][A] -> pi f32 [B][A], v f32 [B][P].  w = 14 device pointers {W0, b0, Wc, bc, Wp, bp, Wfp, bfp, Wv, bv,
   Wf1, bf1, Wf2, bf2}: BatchNorm folded; W0 [9*16][64] and the 2*n_blocks trunk matrices Wc [9*64][64] (row = tap*Cin + ci,
   tap = ky*3 + kx, column = co) in the MFMA fragment order of azg_nn_mb1d_forward, back to back; bc [2*n_blocks][64];
   Wp [64][2], Wfp [50][A] (row = c*25 + cell), Wv [64], Wf1 [25][64], Wf2 [64][P] plain row-major.
   Built for the no-gods geometry (n_blocks = 5, A = 162, P = 2). */
int azg_nn_conv5_forward(const int8_t* boards_dev, const uint8_t* valid_dev, const float* const* w, int n_blocks, int A, int P,
                         int B, float* pi_dev, float* v_dev, void* stream);
/* The same forward with the 2*n_blocks trunk convolutions on split-precision operands: every f32 weight / activation is carried
   as three bf16 numbers (hi + mid + lo = 24 significant bits) and a product is the six bf16 MFMAs of weight >= 2^-24, accumulated
   in f32 (f32-input MFMA runs at 1/16 of the bf16 rate on gfx950; outputs stay within the 1e-5 contract).  Only w[2] differs:
   Wc = [2*n_blocks][4 column tiles][18 K chunks of 32][3 planes hi, mid, lo][64 lanes][8] bf16 with
   element = W_plane[32*chunk + 8*(lane>>4) + j][16*tile + (lane&15)], row index K = tap*64 + ci. */
int azg_nn_conv5_forward_split(const int8_t* boards_dev, const uint8_t* valid_dev, const float* const* w, int n_blocks, int A,
                               int P, int B, float* pi_dev, float* v_dev, void* stream);
/* The same net with the trunk on f16 x 2 split-precision operands (hi = rn16(x), lo = rn16(x - hi): 22 significant bits, three
   v_mfma_f32_16x16x32_f16 per product instead of the six of bf16 x 3; two activation planes per tile holding 64 * x).
   w[2] = the ten 64 -> 64 convolutions as [4 ct][18 chunks][2 planes hi, lo][64 lanes][8] f16 of W * 2^k (one k for the whole net),
   element = W_plane[32*chunk + 8*(lane>>4) + j][16*ct + (lane&15)], K = tap*64 + ci; descale = 2^-k / 64.  Same 1e-5 contract. */
int azg_nn_conv5_forward_h2(const int8_t* boards_dev, const uint8_t* valid_dev, const float* const* w, float descale, int n_blocks,
                            int A, int P, int B, float* pi_dev, float* v_dev, void* stream);
/* The Santorini-with-gods net (nn_version 78, SantoriniNNet.py:167-192,264-271, HeadWithMeta :42-69): two launches on `stream`
   (trunk + value head; policy FC + masked softmax -- the pi rows carry the 132 policy features in between).
   boards int8 [B][5][5][3] (planes 0, 1 = workers / levels, plane 2 = gods and metadata), valid u8 [B][A] -> pi, v.
   w = 19 device pointers {W0, We, be, Wd, bd, Wp, bp, Wm, bm, Whp, bhp, Wfp, bfp, Whv, bhv, Wf1, bf1, Wf2, bf2}: BatchNorm
   folded; W0 [9*16][64], the n_blocks expand matrices We [64][192] and project matrices Wp [192][64] in MFMA fragment order,
   back to back; Wd [n_blocks][192][9] (channel, tap = ky*3 + kx); biases [n_blocks][192 / 192 / 64]; Wm [25][32];
   Whp [64][4], Whv [64][2], Wf1 [82][64], Wf2 [64][P] plain row-major; Wfp [132][A] (rows: channel*25 + cell, then the 32
   metadata features) zero padded to [144][1792] in MFMA fragment order, bfp padded to 1792.  Built for n_blocks = 10, A = 1782, P = 2. */
int azg_nn_s78_forward(const int8_t* boards_dev, const uint8_t* valid_dev, const float* const* w, int n_blocks, int A, int P,
                       int B, float* pi_dev, float* v_dev, void* stream);
/* The same net with the 1x1 convolutions of the trunk on split-precision operands (bf16 x 3, as azg_nn_conv5_forward_split): 8
   samples per workgroup, the expanded tile processed in thirds of 64 channels.  Only w[1] and w[5] differ:
   We / Wp = [n_blocks][3 thirds][4 column tiles][2 K chunks of 32][3 planes hi, mid, lo][64 lanes][8] bf16 with
   element = M_plane[32*chunk + 8*(lane>>4) + j][16*tile + (lane&15)], M = We[:, 64 t .. 64 t + 63] resp. Wp[64 t .. 64 t + 63, :]. */
int azg_nn_s78_forward_split(const int8_t* boards_dev, const uint8_t* valid_dev, const float* const* w, int n_blocks, int A, int P,
                             int B, float* pi_dev, float* v_dev, void* stream);
/* The same with the trunk's 1x1 convolutions and the depthwise pass on f16 x 2 split-precision operands (hi + lo, three
   v_mfma_f32_16x16x32_f16 per product, two planes per tile holding 64 * x): We / Wp = [n_blocks][3 thirds][4 ct][2 chunks]
   [2 planes hi, lo][64 lanes][8] f16 of W * 2^k (one k per family), ds_e / ds_p = 2^-k / 64.  The policy FC runs on the same operands
   (k_s78_policy_h2): w[11] = [112 column tiles][5 K chunks of 32][2 planes hi, lo][64 lanes][8] f16 of Wfp * 2^k (K 132 -> 160,
   N 1782 -> 1792, zero padded; element = W_plane[32*chunk + 8*(lane>>4) + j][16*tile + (lane&15)]) followed by ONE float, its descale
   2^-k / 64 (the 16-byte tail of the buffer).  logits_ws_dev != NULL: three launches -- trunk + value head; the FC as a GEMM (a workgroup =
   64 samples x a quarter of the column tiles: every weight fragment serves four sample groups; raw logits go to logits_ws_dev, [B][1792]
   floats owned by the caller: one per concurrent stream, alive while a captured graph that holds it can be replayed); masked softmax into
   pi.  logits_ws_dev == NULL: FC + softmax in one launch (k_s78_policy_h2, 16 samples per workgroup, no workspace).  Same 1e-5 contract. */
int azg_nn_s78_forward_h2(const int8_t* boards_dev, const uint8_t* valid_dev, const float* const* w, float ds_e, float ds_p, int n_blocks,
                          int A, int P, int B, float* pi_dev, float* v_dev, float* logits_ws_dev, void* stream);
/* The Abalone net (nn_version 21, abalone/AbaloneNNet.py:120-160,173-201; Belgian Daisy): ONE launch on `stream`, 4 samples per
   workgroup (nn_abalone.hip.h).  boards int8 [B][9][9][4] (planes 0, 1 = marbles, 2 = hex mask, 3 = metadata: board[0][0..5][3]),
   valid u8 [B][A] -> pi f32 [B][A] (masked softmax, action = (r*9 + q)*42 + plane), v f32 [B][P] (tanh).
   w = 16 device pointers {W0, b0, We, be, Wd, bd, Wp, bp, Wh, bh, Wm, bm, Wf1, bf1, Wf2, bf2}, BatchNorm folded, f32:
   W0 [2][8][64] = first conv fragment element W0[k = 8*(lane>>4) + m][16*ct + (lane&15)], k = tap*3 + c (zero for k >= 27), b0[24];
   We per block [3][6][64] element We[6*(lane>>4) + m][16*ct + (lane&15)], be [4][48]; Wd [4][48][9], bd [4][48];
   Wp per block [2][12][64] element Wp[12*(lane>>4) + m][16*ct + (lane&15)] (columns >= 24 zero), bp [4][24];
   Wh [3][6][64] = the two head convolutions as one 24 x 48 matrix (columns 0..41 policy, 42..45 value, 46..47 zero), bh [48];
   Wm [6][16], bm[16]; Wf1 [340][64] (row = c*81 + cell, then the 16 meta features), bf1[64]; Wf2 [64][P], bf2[P].
   f32 MFMA operands: the full f32 range, same 1e-5 contract as the torch net.  n_blocks must be 4, A 3402, P 2. */
int azg_nn_aba21_forward(const int8_t* boards_dev, const uint8_t* valid_dev, const float* const* w, int n_blocks, int A, int P, int B,
                         float* pi_dev, float* v_dev, void* stream);
/* The Smallworld net (nn_version 62, smallworld/SmallworldNNet.py:86-180,246-254,268-294; a 3-layer transformer encoder, d_model 48,
   3 heads, feed-forward 192): ONE launch on `stream`, 4 / 3 / 2 samples per workgroup for P = 2 / 3 / 4 (nn_smallworld.hip.h).
   boards int8 [B][N][8] (N = 40 / 52 / 66 tokens), valid u8 [B][A] -> pi f32 [B][A] (masked softmax, A = 5*nA + 16, nA = 23 / 30 / 39
   area tokens), v f32 [B][P] (tanh).  w = 25 device pointers, f32, L = 3 layers; "frag" = MFMA A-operand fragments of W^T [K][Nout],
   element [ct][m][lane] = W^T[16*(m>>2) + 4*(lane>>4) + (m&3)][16*ct + (lane&15)]:
     Tppl [31][48], Tpwr [41][48], Tpl [6][48]   the three embeddings times their out_proj slices (emb @ Wout[:, slice]^T)
     Wst [21][48], bst [48]                       num_proj and bit_proj folded through out_proj: rows x0, x3, x4, x5, x6 (/ 10), bits 0..7
                                                  of x3, bits 0..7 of x4; bias = out_proj.bias + out_proj slices of the two biases
     lnsw, lnsb [48]                              the stem LayerNorm
     Wqkv [L][9][12][64] frag of in_proj_weight^T with the Q columns * 1/4, bqkv [L][144] (Q part * 1/4)
     Wo [L][3][12][64] frag of out_proj, bo [L][48]; ln1w, ln1b [L][48]
     W1 [L][12][12][64] frag of linear1, b1 [L][192]; W2 [L][3][48][64] frag of linear2, b2 [L][48]; ln2w, ln2b [L][48]
     Wl [48][5], bl [5] local head; Wg [48][16], bg [16] global head; Wv [48][P], bv [P] value head.
   f32 MFMA operands: the full f32 range, same 1e-5 contract as the torch net.  n_layers must be 3, (P, A) one of (2, 131), (3, 166),
   (4, 211). */
int azg_nn_sw62_forward(const int8_t* boards_dev, const uint8_t* valid_dev, const float* const* w, int n_layers, int A, int P, int B,
                        float* pi_dev, float* v_dev, void* stream);
/* The Akropolis net (nn_version 31, akropolis/AkropolisNNet.py:91-146,377-388,573-622; pretrained_{2,3,4}pl.pt): ONE launch on `stream`,
   one sample per workgroup of 192 threads (nn_akropolis.hip.h).  boards int8 [B][13][13][3P + 2], valid u8 [B][A] -> pi f32 [B][A]
   (masked softmax, A = 1014 (P + 2), action c*1014 + cell*6 + o), v f32 [B][P] (tanh).  w = 3 device pointers to packed f32 blocks,
   tensors back to back in this order (every BatchNorm folded into the layer before it; CS = P + 2):
     w[0]  Ws [15P][16], bs [16] (dense_scores^T); Wg [2][8], bg [8] (dense_globs); Tc [3][12][32] (embedding through conv1d_constr, per
           position and code), bc [32]; Wi [56][16], bi [16] (proj_i with b1n); Wo [56][96], bo [96] (proj_o^T); Wec [24][32], be [32]
           (proj_p's first 1x1 on the s1 | g1 channels, + its BN shift); Wv1 [56 CS][16], bv1 [16], Wv2 [16][16], bv2 [16], Wv3 [16][P],
           bv3 [P] (value head)
     w[1]  T1 [9 taps][12 codes][8] (embedding through conv1), W1x [9][2][8] (conv1's height / tileID columns), b1 [8]; W2 [9][8 in][8 out],
           b2 [8] (conv2); We [8P][32] (proj_p's first 1x1 on the board channels, player-major)
     w[2]  dws, dwb [32] (depthwise 1x1 + BN), fc1 [32][8], fc1b [8], fc2 [8][32], fc2b [32] (SE), Wp [32][16], bp [16] (project)
   f32 operands, f32 accumulation (the policy dot products in f64).  (P, A) must be (2, 4056), (3, 5070) or (4, 6084). */
int azg_nn_akr31_forward(const int8_t* boards_dev, const uint8_t* valid_dev, const float* const* w, int P, int A, int B, float* pi_dev,
                         float* v_dev, void* stream);
/* The Botanik nets (nn_version 10: botanik/BotanikNNet.py:105-160, 11: :162-237, forward :251-292): ONE launch on `stream`, 8 samples per
   workgroup (nn_botanik.hip.h).  boards int8 [B][66][5][7] (rows 0..25 read), valid u8 [B][428] -> pi f32 [B][428] (masked softmax),
   v f32 [B][2] (tanh).  n_mach = 1 (V10: the 1-d branch and mach0) or 2 (V11: and mach1).  Every BatchNorm folded; f32; the fragment
   element F[k][n] of a [nct][G][64] array sits at lane (n & 15) + 16 * (k / G) of slot (ct, k % G) ("k = G g + m") or, for the streamed
   FC fragments [27][KQ][64], at lane (n & 15) + 16 * (k % 4) of slot (ct, k / 4) ("k = 4 j + g").  w = 10 device pointers:
     w[0] W1d   first_layer_1d W [7][7] (out, in), b [7]; then trunk_1d, output_layers_PI_1d.0, output_layers_V_1d.0, 1629 floats each:
                We [21][7], be [21], Wt [30][30] (depthwise Linear, out, in), sd, bd [21] (its BN), W1 [8][21], b1 [8], W2 [21][8], b2 [21]
                (SE), Wp [7][21], bp [7]
     w[1] Wm    per machine branch 24496 floats: first conv [16][64] (k = 16 g + m, k = tap*7 + c < 63); trunk We [2][4][64], be [32],
                Wd [9][32] (tap-major), bd [32], Wp [1][8][64], bp [16]; six SE blocks (policy head 0..2, value head 0..2) of 3680:
                We [3][4][64], be [48], Wd [9][48], bd [48], W1 [16][48], b1 [16], W2 [48][16], b2 [48], Wp [1][12][64], bp [16]
     w[2] Wpi   the branch policy Linears stacked along K: [27][53][64] (1-d, K 210 padded to 212), then [27][196][64] per branch
     w[3] bpi   [432] their biases summed; w[4] Wv: the branch value Linears, [2][210] then [2][784] per branch
     w[5..8]    final_layers_PI.0 / .2: [27][108][64] (K and N padded to 432), bias [432] each
     w[9] tail  [14]: the branch value biases summed [2], final_layers_V.0 W [2][2], b [2], final_layers_V.2 W [2][2], b [2]
   Same 1e-5 contract as the torch net.  n_mach must be 1 or 2, P 2, A 428. */
int azg_nn_bot_forward(const int8_t* boards_dev, const uint8_t* valid_dev, const float* const* w, int n_mach, int P, int A, int B,
                       float* pi_dev, float* v_dev, void* stream);

/* ---- measurement helpers ---- */
/* time `iters` back-to-back launches of kernel `which` (0 = select, 1 = expand_backup) with hipEvents on `stream`
   (state is mutated like normal rounds); returns average milliseconds per launch. */
int azg_forest_last_kernel_ms(azg_forest* f, int which, double* avg_ms, uint64_t* launches);
int azg_forest_enable_timing(azg_forest* f, int enable);
/* args.numMCTSSims / args.prob_fullMCTS for the searches that BEGIN after this call (MCTS.py:58-59 reads both at every
   getActionProb call); searches in flight keep their size.  Both are kernel arguments: HIP graphs that captured this forest's
   launches must be captured again (SelfPlayEngine.set_search_params does). */
int azg_forest_set_search_params(azg_forest* f, int numMCTSSims, double prob_fullMCTS);

#ifdef __cplusplus
}
#endif
#endif
