!  prcp_indices_driver.f90 -- TEST INFRASTRUCTURE, not product code.
!
!  A bind(C) driver over the UNMODIFIED reference module mw_forcing_statistic, compiled by tests/golden/make_prcp_indices.py
!  against the module files and objects the oracle recipe leaves in oracle/_ref/obj_parity (same flags: -O2 -ffp-contract=off).
!  It fills SetupDT / MeshDT / Input_DataDT from flat arrays the way tests/golden/mean_forcing_driver.f90 does, calls the
!  reference's compute_prcp_indices (smash/solver/routine/mw_forcing_statistic.f90:77-220) on the caller's (4, ng, nt) array,
!  which the routine updates in place.
!
!  This file is ours; it contains no reference source text.  Nothing compiled from it is committed.

module prcp_indices_driver

    use iso_c_binding
    use md_constant
    use mwd_setup
    use mwd_mesh
    use mwd_input_data
    use mw_sparse_storage
    use mw_forcing_statistic, only: compute_prcp_indices

    implicit none

contains

    !  icfg = (nrow; ncol; nt; ng; sparse_storage 0/1)
    !  arrays column-major as the reference holds them, path and gauge_pos 1-based
    subroutine pi_run(icfg, flwdir, path, active_cell, gauge_pos, flwdst, prcp, prcp_indices) bind(C, name="pi_run")

        integer(c_int), intent(in) :: icfg(5)
        integer(c_int), intent(in) :: flwdir(icfg(1), icfg(2)), path(2, icfg(1)*icfg(2)), active_cell(icfg(1), icfg(2))
        integer(c_int), intent(in) :: gauge_pos(icfg(4), 2)
        real(c_float), intent(in) :: flwdst(icfg(1), icfg(2)), prcp(icfg(1), icfg(2), icfg(3))
        real(c_float), intent(inout) :: prcp_indices(4, icfg(4), icfg(3))

        type(SetupDT) :: setup
        type(MeshDT) :: mesh
        type(Input_DataDT) :: input_data
        integer :: nrow, ncol, nt, ng, t

        nrow = icfg(1); ncol = icfg(2); nt = icfg(3); ng = icfg(4)
        setup%structure = "gr-b"
        setup%sparse_storage = (icfg(5) .ne. 0)
        setup%ntime_step = nt
        call SetupDT_initialise(setup, 0, ng)

        call MeshDT_initialise(mesh, setup, nrow, ncol, ng)
        mesh%flwdir = flwdir
        mesh%flwdst = flwdst
        mesh%path = path
        mesh%active_cell = active_cell
        mesh%gauge_pos = gauge_pos
        mesh%nac = count(active_cell .eq. 1)
        if (setup%sparse_storage) call compute_rowcol_to_ind_sparse(mesh)

        call Input_DataDT_initialise(input_data, setup, mesh)
        if (setup%sparse_storage) then
            do t = 1, nt
                call sparse_matrix_to_vector_r(mesh, prcp(:, :, t), input_data%sparse_prcp(:, t))
            end do
        else
            input_data%prcp = prcp
        end if

        call compute_prcp_indices(setup, mesh, input_data, prcp_indices)

    end subroutine pi_run

end module prcp_indices_driver
